// Front end of the hand-written axis passes: routes every call to the family of its line length (fft_kernels.hip is
// compiled once per family: power-of-two lines, lines with one factor 3, lines with one factor 5).
#include "pruned.hpp"
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <set>

namespace lsfc {

void warmup_pointwise(); void warmup_krylov_blas(); void warmup_symbol(); void warmup_precond(); void warmup_trisolve(); void warmup_blocktri(); void warmup_receivers();      // pointwise.hip, krylov_blas.hip, symbol.hip, precond.hip, trisolve.hip, blocktri.hip, receivers.hip
extern const PrunedFamily pruned_family_f2, pruned_family_f3, pruned_family_f5;     // fft_kernels.hip, one per compilation

// 2: L = 2^k (32..2048);  3: L = 3 * 2^k (48..1536);  5: L = 5 * 2^k (80..1280);  0: not supported
static int family(int64_t L) {
    if (L < 32 || L > 2048) return 0;
    int64_t v = L; while (v % 2 == 0) v /= 2;
    if (v == 1) return 2;
    if (v == 3) return L >= 48 && L <= 1536 ? 3 : 0;
    if (v == 5) return L >= 80 && L <= 1280 ? 5 : 0;
    return 0;
}
bool pruned_length_supported(int64_t L) { return family(L) != 0; }
static const PrunedFamily& family_of(int64_t L) {
    switch (family(L)) {
    case 2: return pruned_family_f2;
    case 3: return pruned_family_f3;
    case 5: return pruned_family_f5;
    default: fail(LSFC_EINVAL, "pruned pipeline: unsupported padded length %d", (int)L);
    }
}

void pruned_warmup(int device) {
    static std::mutex mu;
    static std::set<int> done;
    std::lock_guard<std::mutex> lock(mu);
    if (done.count(device)) return;
    // LSFC_EAGER_LOAD=0 (developer switch, diagnostics only): leave the code objects to HIP's lazy loading at first launch
    if (const char* e = getenv("LSFC_EAGER_LOAD")) if (e[0] == '0') return;
    pruned_family_f2.warmup(); pruned_family_f3.warmup(); pruned_family_f5.warmup();
    warmup_pointwise(); warmup_krylov_blas(); warmup_symbol(); warmup_precond(); warmup_trisolve(); warmup_blocktri(); warmup_receivers();
    LSFC_HIP(hipDeviceSynchronize());
    done.insert(device);
}

int pruned_best_length(int64_t n) {
    // LSFC_POW2_ONLY=1 (developer switch): power-of-two lines only, for A/B timing of the mixed-radix lines
    const char* e = getenv("LSFC_POW2_ONLY");
    const bool pow2_only = e && e[0] == '1';
    for (int64_t L = (2 * n > 32 ? 2 * n : 32); L <= 2048; ++L) if (family(L) && (!pow2_only || family(L) == 2)) return (int)L;
    return 0;
}

// LSFC_DEBUG_SYNC=1 (developer switch): synchronise the device after every pass and name the pass that failed -- turns an
// asynchronous GPU fault or launch error into an error message at the kernel that caused it
static bool debug_sync() { static const bool on = getenv("LSFC_DEBUG_SYNC") && getenv("LSFC_DEBUG_SYNC")[0] == '1'; return on; }
static void debug_check(const char* pass, int L) {
    if (!debug_sync()) return;
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) { (void)hipGetLastError(); fail(LSFC_EHIP, "%s (line length %d) failed: %s", pass, L, hipGetErrorString(e)); }
    fprintf(stderr, "[lsfc debug] %s L=%d ok\n", pass, L);
}
static void require_batch(int nrhs) {
    LSFC_REQUIRE(nrhs >= 1 && nrhs <= LSFC_MAX_BATCH, "batch of %d right-hand sides (1..%d per launch)", nrhs, LSFC_MAX_BATCH);
}
void pruned_xfwd(const PrunedTuning& tn, const XPass& a, hipStream_t st) { require_batch(a.nrhs); family_of(a.L).xfwd(tn, a, st); debug_check("pruned_xfwd", a.L); }
void pruned_xinv(const PrunedTuning& tn, const XPass& a, hipStream_t st) { require_batch(a.nrhs); family_of(a.L).xinv(tn, a, st); debug_check("pruned_xinv", a.L); }
void pruned_yfwd(const PrunedTuning& tn, const YPass& a, hipStream_t st) { family_of(a.L).yfwd(tn, a, st); debug_check("pruned_yfwd", a.L); }
void pruned_yinv(const PrunedTuning& tn, const YPass& a, hipStream_t st) { family_of(a.L).yinv(tn, a, st); debug_check("pruned_yinv", a.L); }
void pruned_zfused(const PrunedTuning& tn, const FusedPass& a, hipStream_t st) { family_of(a.L).zfused(tn, a, st); debug_check("pruned_zfused", a.L); }
// the descriptions: pure host arithmetic, no launch (and no debug synchronisation)
PassForm pruned_xfwd_form(const PrunedTuning& tn, const XPass& a) { return family_of(a.L).xform(PassFamily::XFWD, tn, a); }
PassForm pruned_xinv_form(const PrunedTuning& tn, const XPass& a) { return family_of(a.L).xform(PassFamily::XINV, tn, a); }
PassForm pruned_yfwd_form(const PrunedTuning& tn, const YPass& a) { return family_of(a.L).yform(PassFamily::YFWD, tn, a); }
PassForm pruned_yinv_form(const PrunedTuning& tn, const YPass& a) { return family_of(a.L).yform(PassFamily::YINV, tn, a); }
PassForm pruned_zfused_form(const PrunedTuning& tn, const FusedPass& a) { return family_of(a.L).zfused_form(tn, a); }
const char* pass_family_name(PassFamily fam) {
    switch (fam) {
    case PassFamily::XFWD: return "xfwd";
    case PassFamily::XINV: return "xinv";
    case PassFamily::YFWD: return "yfwd";
    case PassFamily::YINV: return "yinv";
    case PassFamily::ZFUSED: return "zfused";
    case PassFamily::ZFUSED_HALF: return "zfused_half";
    case PassFamily::ZFUSED_PERSIST: return "zfused_persist";
    case PassFamily::ZFUSED_PERSIST_HALF: return "zfused_persist_half";
    }
    return "?";
}
int pass_form_print(const PassForm& f, char* buf, size_t cap) {
    const bool xpass = f.family == PassFamily::XFWD || f.family == PassFamily::XINV;
    const bool ypass = f.family == PassFamily::YFWD || f.family == PassFamily::YINV;
    int k = snprintf(buf, cap, "%s L=%d SPLIT=%d FULL=%d", pass_family_name(f.family), f.L, (int)f.split, (int)f.full);
    auto more = [&](const char* fmt, auto... a) { if (k >= 0 && (size_t)k < cap) k += snprintf(buf + k, cap - (size_t)k, fmt, a...); };
    if (!xpass) more(" LINES=%d WPE=%d", f.lines, f.wpe);
    if (ypass) more(" FORCED_SPLIT=%d TG=%d TZ=%d", (int)f.forced_split, f.tg, f.tz);
    if (!xpass && !ypass) more(" PREFETCH=%d ZE=%d TWL=%d BATCH=%d LATE_SYM=%d TICKETS=%d XL=%d PER_MEMBER=%d", (int)f.prefetch, (int)f.ze, (int)f.twl,
                                 (int)f.batch, (int)f.late_sym, (int)f.tickets, f.xl, (int)f.per_member);
    return k;
}

void pruned_perm(int L, int* freq_of_storage) { family_of(L).perm(L, freq_of_storage); }
int pruned_twfull_len(int L) { return family_of(L).twfull_len(L); }
void pruned_twfull(int L, const cplx* tw, cplx* out) { family_of(L).twfull(L, tw, out); }

static bool env_flag(const char* name, bool dflt) {
    const char* v = getenv(name);
    if (!v || !*v) return dflt;
    return v[0] == '1' || v[0] == 'y' || v[0] == 't';
}

PrunedTuning pruned_default_tuning() {
    PrunedTuning t;
    for (const TuningKnob& k : TUNING_KNOBS) {
        if (k.flag) t.*k.flag = env_flag(k.env, t.*k.flag);
        else if (const char* v = getenv(k.env)) t.*k.value = atoi(v);
    }
    return t;
}

} // namespace lsfc
