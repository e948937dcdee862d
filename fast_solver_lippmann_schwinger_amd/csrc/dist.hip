// Slab-distributed 3D operator: one process per GPU, RCCL over xGMI.
//
// Rank p owns z planes [p*lz, (p+1)*lz) of x, y and nu.  Per apply:
//   phase 1 (local)   k_xfwd on the own planes; the output is written already packed per destination
//                     rank: S1[q][W][m][lz], W = Lx/P storage indices of x' for rank q
//   exchange 1        all-to-all (grouped ncclSend/ncclRecv): block q of S1 -> rank q.  The received blocks,
//                     ordered by source rank, ARE the natural array R1[W][m][l] (blocks concatenate along z)
//   phase 2 (local)   k_yfwd, k_zfused (symbol slab of the own x' tiles), k_yinv on R1 / A2
//   exchange 2        block p of R1 (z range of rank p) -> rank p, received into S1[q][W][m][lz]
//   phase 3 (local)   k_xinv reads that packed layout directly, y = alpha*x + beta*(.)
// No pack/unpack/transposition kernel runs: the chunked addressing of the x passes does the packing,
// and the exchange moves 2N complex per transpose, the minimum-volume point of the pipeline.
#include "plan.hpp"
#include "apply.hpp"
#include "pointwise.hpp"
#include "dist_schedule.hpp"
#include "team.hpp"
#include <rccl/rccl.h>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace lsfc {

#define LSFC_NCCL(expr) do { ncclResult_t r_ = (expr); if (r_ != ncclSuccess) \
    ::lsfc::fail(LSFC_EHIP, "%s failed: %s (%s:%d)", #expr, ncclGetErrorString(r_), __FILE__, __LINE__); } while (0)

DistState::~DistState() {
    for (auto& v : { &ev_in, &ev_done, &ev_back }) for (hipEvent_t e : *v) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : { ev_p1, ev_p1a, ev_backa }) if (e) (void)hipEventDestroy(e);
    if (cs1) (void)hipStreamDestroy(cs1);
    if (cs2) (void)hipStreamDestroy(cs2);
    if (st2) (void)hipStreamDestroy(st2);
    if (comm2) (void)ncclCommDestroy((ncclComm_t)comm2);
    if (comm) (void)ncclCommDestroy((ncclComm_t)comm);
}

// block of one (rank, chunk) pair in S1 / R1: [Wc][m][lz]
static int64_t block_elems(const lsfc_plan* p) { return (int64_t)p->dist->Wc * p->dims[1] * p->dist->lz; }

// The x passes on the own planes (part = -1), or on their lower / upper half (0 / 1: the z halves of every S1 block): lines of S1
// in blocks [Wc][m][lz].  x, y: the rank's vectors (y null for the forward pass).  M and the bare convolution only (a real nu on
// the input side, no conjugation: plan.hpp, conv_forward_only)
static XPass slab_xpass(const lsfc_plan* p, const cplx* x, cplx* y, bool use_nu, double alpha, double beta, int part) {
    const DistState* d = p->dist.get();
    const int64_t all = (int64_t)p->dims[1] * d->lz, nl = part < 0 ? all : all / 2, l0 = part == 1 ? all / 2 : 0;
    const int64_t off = l0 * p->dims[0];            // the part's first line in the vectors and in nu
    VecBatch vb{}; vb.x[0] = x + off; if (y) vb.y[0] = y + off;
    // chunk width Wc: storage index s of a line lands in block s / Wc = dest_rank * K + chunk
    return XPass{.L = p->pads[0], .vb = vb, .nrhs = 1, .work = d->S1.p + l0 * d->Wc, .wbatch = 0, .tw = p->tw[0].p, .nlines = nl, .W = d->Wc, .Wp = d->Wc,
                 .n = p->dims[0], .bstride = all * d->Wc, .nu = NuPlanes{use_nu ? p->nu.p + off : nullptr, nullptr}, .conj = false, .alpha = alpha, .beta = beta};
}
static void phase1(lsfc_plan* p, const cplx* x, bool use_nu, hipStream_t st, int part = -1) {
    pruned_xfwd(p->tuning, slab_xpass(p, x, nullptr, use_nu, 0.0, 0.0, part), st);
}
// the y passes of chunk c: R1 chunk [m][l][Wc] <-> the chunk's tiles of A2
static YPass chunk_ypass(const lsfc_plan* p, int c) {
    const DistState* d = p->dist.get();
    const int m = p->dims[1], l = p->dims[2];
    return YPass{.L = p->pads[1], .a1 = d->R1.p + (int64_t)c * d->Wc * m * l, .a2 = p->A2.p + (int64_t)c * (d->Wc / 8) * p->pads[1] * p->pitch2, .tw = p->tw[1].p,
                 .Lx = d->Wc, .m = m, .l = l, .p1 = d->Wc, .p2 = p->pitch2, .nrhs = 1, .batch1 = 0, .batch2 = 0};
}
static void phase2_yfwd(lsfc_plan* p, int c, hipStream_t st) { pruned_yfwd(p->tuning, chunk_ypass(p, c), st); }
static void phase2_zfused(lsfc_plan* p, int c, hipStream_t st) {
    const DistState* d = p->dist.get();
    plan_zfused_3d(p, d->Wc, (int64_t)c * (d->Wc / 8) * p->pads[1] * p->pitch2, (int64_t)c * d->Wc * p->sym_rows * p->sym_hz, 1, st);
}
static void phase2_yinv(lsfc_plan* p, int c, hipStream_t st) { pruned_yinv(p->tuning, chunk_ypass(p, c), st); }
static void phase2(lsfc_plan* p, int c, hipStream_t st) { phase2_yfwd(p, c, st); phase2_zfused(p, c, st); phase2_yinv(p, c, st); }
static void phase3(lsfc_plan* p, const cplx* x, cplx* y, double alpha, double beta, hipStream_t st, int part = -1) {
    pruned_xinv(p->tuning, slab_xpass(p, x, y, false, alpha, beta, part), st);
}

// The ranks this process drives: one rank of a multi-process plan (the plan itself, with the communicators of its DistState) or
// all P sub-plans of a multi-device plan (MultiState's communicators, or the copy transport).  A stream of one device may wait
// on an event of another, so one host thread enqueues the same schedule (dist_schedule.hpp) either way.
namespace {
using dsched::Lane; using dsched::Ev; using dsched::Op; using dsched::Step;
struct Local {
    std::vector<lsfc_plan*> plan;       // plan[i]->dist->rank is the rank; a multi-device plan drives them all, in rank order
    int P, K;                           // ranks of the whole job, pipeline chunks
    bool rccl;                          // blocks between different ranks: one RCCL group over the local ranks' message lists, or source-issued copies
    bool force_comm = false;            // one rank, the self block sent through RCCL (LSFC_DIST_FORCE_COMM)
    bool set_device = false;            // multi-device: the rank's device is made current before anything is enqueued for it
    void* const* comm = nullptr; void* const* comm2 = nullptr;    // per local rank: way in / way back

    explicit Local(lsfc_plan* p) {
        if (p->multi) {
            MultiState* ms = p->multi.get();
            for (auto& sp : ms->sub) plan.push_back(sp.get());
            rccl = ms->rccl; set_device = true; comm = ms->comm.data(); comm2 = ms->comm2.data();
        } else {
            plan.push_back(p);
            rccl = true; force_comm = p->dist->force_comm; comm = &p->dist->comm; comm2 = &p->dist->comm2;
        }
        P = d(0)->nranks; K = d(0)->K;
    }
    int n() const { return (int)plan.size(); }
    DistState* d(int i) const { return plan[(size_t)i]->dist.get(); }
    void dev(int i) const { if (set_device) LSFC_HIP(hipSetDevice(plan[(size_t)i]->device)); }
    template <class F> void each(F&& f) const { for (int i = 0; i < n(); ++i) { dev(i); f(i); } }
    hipStream_t stream(int i, Lane on) const {
        return on == Lane::COMPUTE ? plan[(size_t)i]->stream : on == Lane::COMPUTE2 ? d(i)->st2 : on == Lane::IN ? d(i)->cs1 : d(i)->cs2;
    }
    hipEvent_t event(int i, Ev ev, int c) const {
        DistState* s = d(i);
        switch (ev) {
            case Ev::P1A: return s->ev_p1a; case Ev::P1: return s->ev_p1; case Ev::BACKA: return s->ev_backa;
            case Ev::IN: return s->ev_in[(size_t)c]; case Ev::DONE: return s->ev_done[(size_t)c]; default: return s->ev_back[(size_t)c];
        }
    }
};

// Exchange of chunk c over the local ranks, on their streams `on`.
//   way in  : S1 block (q, c)  -> rank q, lands in R1 slot (c, <source rank>)
//   way back: R1 slot (c, q)   -> rank q, lands in S1 block (<source rank>, c)
// part = -1: whole blocks; 0 / 1: their lower / upper z halves (blocks are [z][m][Wc], z slowest: halves are contiguous).
// Every rank's message list -- peers, order, offsets -- is dist_schedule.hpp's, checked on the CPU for P = 2, 4, 8: the self
// block first, a device copy; then the pairwise steps, as sends and receives of one RCCL group or, with all ranks local, as
// copies issued by the source (copy engines instead of CUs; every source starts with a different peer).
void exchange(const Local& L, int c, bool back, int part, Lane on) {
    const int n = L.n(), P = L.P;
    std::vector<std::vector<dsched::Msg>> msgs((size_t)n);
    for (int i = 0; i < n; ++i) msgs[(size_t)i] = dsched::exchange_messages(L.d(i)->rank, P, L.K, c, back, part, block_elems(L.plan[0]));
    auto ptr = [&](int i, const dsched::Msg& m) { return (m.in_s1 ? L.d(i)->S1.p : L.d(i)->R1.p) + m.off; };
    auto comm = [&](int i) { return (ncclComm_t)(back ? L.comm2[i] : L.comm[i]); };
    auto post = [&](int i, const dsched::Msg& m) {
        if (m.send) LSFC_NCCL(ncclSend(ptr(i, m), (size_t)m.count * 2, ncclDouble, m.peer, comm(i), L.stream(i, on)));
        else LSFC_NCCL(ncclRecv(ptr(i, m), (size_t)m.count * 2, ncclDouble, m.peer, comm(i), L.stream(i, on)));
    };
    if (L.force_comm && P == 1) {
        // single-rank exercise of the RCCL path: the self block travels through ncclSend/ncclRecv
        LSFC_NCCL(ncclGroupStart());
        post(0, msgs[0][0]); post(0, msgs[0][1]);
        LSFC_NCCL(ncclGroupEnd());
        return;
    }
    L.each([&](int i) {
        LSFC_HIP(hipMemcpyAsync(ptr(i, msgs[(size_t)i][1]), ptr(i, msgs[(size_t)i][0]), (size_t)msgs[(size_t)i][0].count * sizeof(cplx), hipMemcpyDeviceToDevice, L.stream(i, on)));
    });
    if (P == 1) return;
    if (L.rccl) {
        LSFC_NCCL(ncclGroupStart());
        for (int i = 0; i < n; ++i) for (size_t k = 2; k < msgs[(size_t)i].size(); ++k) post(i, msgs[(size_t)i][k]);
        LSFC_NCCL(ncclGroupEnd());
        return;
    }
    // (all ranks are local, i == rank: the send of step s to q = r + s lands where q's receive of step s, from r, points)
    L.each([&](int r) {
        for (int s = 1; s < P; ++s) {
            const dsched::Msg& snd = msgs[(size_t)r][(size_t)(2 * s)];
            const int q = snd.peer, dq = L.plan[(size_t)q]->device, dr = L.plan[(size_t)r]->device;
            cplx* dst = ptr(q, msgs[(size_t)q][(size_t)(2 * s + 1)]);
            const size_t bytes = (size_t)snd.count * sizeof(cplx);
            if (dq == dr) LSFC_HIP(hipMemcpyAsync(dst, ptr(r, snd), bytes, hipMemcpyDeviceToDevice, L.stream(r, on)));
            else LSFC_HIP(hipMemcpyPeerAsync(dst, dq, ptr(r, snd), dr, bytes, L.stream(r, on)));
        }
    });
}

// The overlapped apply: dist_schedule.hpp's steps (pipeline_steps, in the order of issue) on the streams and events of the local
// ranks.  x[i], y[i]: the vectors of local rank i.  host_sync (the multi-device plan under LSFC_DIST_OVERLAP=0): the host waits
// for the passes of a chunk on every rank before its way back is enqueued.
struct Pipeline {
    const Local& L; const cplx* const* x; cplx* const* y; bool use_nu; double alpha, beta; bool host_sync;
    int current = -1;                   // the device this apply made current last (-1: not known), so that it is set once per change
    void dev(int i) {
        const int want = L.plan[(size_t)i]->device;
        if (L.set_device && want != current) { LSFC_HIP(hipSetDevice(want)); current = want; }
    }
    void begin(const Step& s) {
        if (!host_sync || s.op != Op::EXCH_BACK) return;
        L.each([&](int i) { LSFC_HIP(hipStreamSynchronize(L.plan[(size_t)i]->stream)); if (L.d(i)->st2) LSFC_HIP(hipStreamSynchronize(L.d(i)->st2)); });
        current = -1;
    }
    void wait(int i, Lane on, int q, Ev ev, int c) { dev(i); LSFC_HIP(hipStreamWaitEvent(L.stream(i, on), L.event(q, ev, c), 0)); }
    void record(int i, Lane on, Ev ev, int c) { dev(i); LSFC_HIP(hipEventRecord(L.event(i, ev, c), L.stream(i, on))); }
    void run(int i, const Step& s) {
        dev(i);
        lsfc_plan* p = L.plan[(size_t)i];
        if (s.op == Op::XFWD) phase1(p, x[i], use_nu, L.stream(i, s.on), s.part);
        else if (s.op == Op::PASSES) phase2(p, s.c, L.stream(i, s.on));
        else phase3(p, x[i], y[i], alpha, beta, L.stream(i, s.on), s.part);
    }
    void exchange(const Step& s) { lsfc::exchange(L, s.c, s.op == Op::EXCH_BACK, s.part, s.on); current = -1; }
};
void pipelined_convolve(const Local& L, const cplx* const* x, cplx* const* y, const ConvOp& op, bool edges, bool host_sync) {
    Pipeline sink{L, x, y, op.nu == NuSide::INPUT, op.alpha, op.beta, host_sync};
    dsched::issue(dsched::pipeline_steps(L.K, edges, L.d(0)->st2 != nullptr), L.n(), sink);
}

// The seven stages of one apply, un-overlapped, each on the compute streams of all local ranks: name, bytes moved per rank
// (N = local points, 16 B each) and what runs.  exchanges = false (simulated ranks, which have nobody to exchange with): the
// compute stages only.
struct Stage { const char* name; double bytes; std::function<void()> run; };
std::vector<Stage> apply_stages(const Local& L, std::vector<const cplx*> x, std::vector<cplx*> y, bool exchanges) {
    const double N = (double)L.plan[0]->N, C = 16.0, om2 = L.plan[0]->omega * L.plan[0]->omega;
    const int K = L.K;
    auto st = [L](int i) { return L.stream(i, Lane::COMPUTE); };
    auto chunks = [L, K, st](void (*pass)(lsfc_plan*, int, hipStream_t)) { return [=] { L.each([&](int i) { for (int c = 0; c < K; ++c) pass(L.plan[(size_t)i], c, st(i)); }); }; };
    auto alltoall = [L, K](bool back) { return [=] { for (int c = 0; c < K; ++c) exchange(L, c, back, -1, Lane::COMPUTE); }; };
    std::vector<Stage> s;
    s.push_back({"xfwd", N * (C + 8) + 2 * N * C, [=] { L.each([&](int i) { phase1(L.plan[(size_t)i], x[(size_t)i], true, st(i)); }); }});
    if (exchanges) s.push_back({"alltoall_in", 2 * N * C, alltoall(false)});
    s.push_back({"yfwd", 6 * N * C, chunks(phase2_yfwd)});
    s.push_back({"zfused", 16 * N * C, chunks(phase2_zfused)});
    s.push_back({"yinv", 6 * N * C, chunks(phase2_yinv)});
    if (exchanges) s.push_back({"alltoall_back", 2 * N * C, alltoall(true)});
    s.push_back({"xinv", 4 * N * C, [=] { L.each([&](int i) { phase3(L.plan[(size_t)i], x[(size_t)i], y[(size_t)i], 1.0, om2, st(i)); }); }});
    return s;
}
} // namespace

void dist_convolve_dev(lsfc_plan* p, const cplx* x, cplx* y, const ConvOp& op) {
    LSFC_REQUIRE(conv_forward_only(op), "the transposed and the adjoint operator are not available on a distributed plan");
    DistState* d = p->dist.get();
    LSFC_REQUIRE(!d->sim, "simulated ranks are driven through lsfc_dist_sim_apply");
    LSFC_REQUIRE(!d->member, "the ranks of a multi-device plan are driven through their parent plan");
    const Local L(p);
    // LSFC_DIST_OVERLAP=0: no overlap -- every exchange on the compute stream, chunk after chunk (debugging aid)
    if ((d->nranks == 1 && !d->force_overlap) || d->no_overlap) {
        hipStream_t st = p->stream;
        phase1(p, x, op.nu == NuSide::INPUT, st);
        for (int c = 0; c < d->K; ++c) { exchange(L, c, false, -1, Lane::COMPUTE); phase2(p, c, st); exchange(L, c, true, -1, Lane::COMPUTE); }
        phase3(p, x, y, op.alpha, op.beta, st);
        return;
    }
    // software pipeline over the K chunks of the owned x' range: the all-to-all of chunk c+1 (stream cs1) and the
    // all-to-all back of chunk c-1 (stream cs2, second communicator) run while chunk c is transformed
    pipelined_convolve(L, &x, &y, op, d->split_edges && d->lz % 2 == 0, false);
}

void dist_allreduce_sum(lsfc_plan* p, cplx* dev, int count) {
    DistState* d = p->dist.get();
    if (!d || d->sim || d->member || (d->nranks == 1 && !d->force_comm)) return;
    LSFC_NCCL(ncclAllReduce(dev, dev, (size_t)count * 2, ncclDouble, ncclSum, (ncclComm_t)d->comm, p->stream));
}

void dist_profile_stages(lsfc_plan* p, const cplx* x, cplx* y, std::function<void(const char*, double, std::function<void()>)> add) {
    DistState* d = p->dist.get();
    // un-overlapped, stage by stage, all on the plan's stream (the production path overlaps the exchanges)
    const bool sim = d->sim || d->member;                       // simulated rank: compute stages only (per-rank kernel times at P ranks)
    if (sim) {
        // no exchange runs here, so the receive buffer would hold the zeros of plan creation and the y / z / y passes would
        // transform zeros -- on which this power-limited chip clocks ~9 % higher.  Prime it once with the x pass's own
        // output (same size: P * K blocks either way), i.e. with data of the statistics the real exchange delivers.
        phase1(p, x, true, p->stream);
        LSFC_HIP(hipMemcpyAsync(d->R1.p, d->S1.p, std::min(d->R1.bytes(), d->S1.bytes()), hipMemcpyDeviceToDevice, p->stream));
    }
    for (Stage& s : apply_stages(Local(p), {x}, {y}, !sim)) add(s.name, s.bytes, std::move(s.run));
}

// ---------------------------------------------------------------------------
static void create_dist_plan(lsfc_plan** out, int64_t n, int64_t m, int64_t l, double box, double omega, const double* nu_local,
                             unsigned flags, int device, int rank, int nranks, const unsigned char* id, bool sim, bool member = false) {
    LSFC_REQUIRE(out, "NULL argument"); *out = nullptr;
    LSFC_REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, "bad rank %d of %d", rank, nranks);
    LSFC_REQUIRE(n % 2 == 0 && m % 2 == 0 && l % 2 == 0, "even grid sizes only");
    LSFC_REQUIRE(l % nranks == 0, "l = %lld is not divisible by the number of ranks %d", (long long)l, nranks);
    for (int64_t v : { n, m, l }) LSFC_REQUIRE(pruned_best_length(v) != 0 && pruned_best_length(v) <= 4 * v, "distributed plan: grid sizes from 8 to 1024 per axis");
    LSFC_REQUIRE((pruned_best_length(n) / 8) % nranks == 0 && is_pow2(nranks),
                 "number of ranks must be a power of two dividing Lx/8 (Lx = %d is the padded line length for n = %lld)", pruned_best_length(n), (long long)n);
    std::unique_ptr<lsfc_plan> p(new lsfc_plan());
    const int lz = (int)(l / nranks);
    // local nu: n*m*lz doubles
    plan_common_init(p.get(), 3, n, m, lz, nu_local, omega, LSFC_QUAD_GREENGARD_VICO, flags & ~LSFC_FLAG_LITERAL_PAD, device);
    p->dims[2] = (int)l;                            // dims are global; N stays local
    p->N = n * m * lz;
    for (int d = 0; d < 3; ++d) { p->pads[d] = pruned_best_length(p->dims[d]); p->crop[d] = 0; }
    p->dist.reset(new DistState());
    DistState* d = p->dist.get();
    d->rank = rank; d->nranks = nranks; d->sim = sim; d->member = member; d->lz = lz; d->W = p->pads[0] / nranks;
    // pipeline chunks: up to 4, each at least one 8-wide tile (LSFC_DIST_CHUNKS overrides; 1 disables the overlap)
    int K = 4;
    if (const char* v = getenv("LSFC_DIST_CHUNKS")) K = atoi(v);
    if (nranks == 1 && !sim && !getenv("LSFC_DIST_CHUNKS") && !getenv("LSFC_DIST_FORCE_OVERLAP")) K = 1;
    const dsched::Chunks ch = dsched::plan_chunks(p->pads[0], nranks, K);
    K = ch.K; d->K = ch.K; d->Wc = ch.Wc;
    // LSFC_DIST_FORCE_OVERLAP=1: run the three-stream pipeline even with one rank (tests of the event logic)
    d->force_overlap = getenv("LSFC_DIST_FORCE_OVERLAP") && getenv("LSFC_DIST_FORCE_OVERLAP")[0] == '1';
    // LSFC_DIST_OVERLAP=0: every exchange on the compute stream; LSFC_DIST_SPLIT_EDGES=0: no z-half split of the pipeline ends
    d->no_overlap = getenv("LSFC_DIST_OVERLAP") && getenv("LSFC_DIST_OVERLAP")[0] == '0';
    d->split_edges = !(getenv("LSFC_DIST_SPLIT_EDGES") && getenv("LSFC_DIST_SPLIT_EDGES")[0] == '0');
    // LSFC_DIST_FORCE_COMM=1: build the communicators and route the (self) exchange through RCCL even with one rank
    d->force_comm = !sim && !member && getenv("LSFC_DIST_FORCE_COMM") && getenv("LSFC_DIST_FORCE_COMM")[0] == '1';
    if (member) d->force_overlap = false;               // the parent plan drives the streams of its ranks
    if (!sim && !member && (nranks > 1 || d->force_comm)) {
        LSFC_REQUIRE(id, "NULL unique id");
        // an all-zero id means the caller never received rank 0's id (no broadcast happened): ncclCommInitRank would
        // block forever on every rank instead of failing
        bool nonzero = false;
        for (int i = 0; i < LSFC_UNIQUE_ID_BYTES; ++i) nonzero = nonzero || id[i] != 0;
        LSFC_REQUIRE(nonzero, "the RCCL unique id is all zeros: ship the bytes of lsfc_dist_unique_id() from rank 0 to every rank first");
        ncclUniqueId uid; static_assert(sizeof(uid) == LSFC_UNIQUE_ID_BYTES, "unique id size");
        memcpy(&uid, id, sizeof uid);
        ncclComm_t comm, comm2;
        LSFC_NCCL(ncclCommInitRank(&comm, nranks, uid, rank));
        d->comm = comm;
        LSFC_NCCL(ncclCommSplit(comm, 0, rank, &comm2, nullptr));
        d->comm2 = comm2;
    }
    if (!sim && (nranks > 1 || d->force_overlap || member)) {
        LSFC_HIP(hipStreamCreateWithFlags(&d->cs1, hipStreamNonBlocking));
        LSFC_HIP(hipStreamCreateWithFlags(&d->cs2, hipStreamNonBlocking));
        // LSFC_DIST_COMPUTE_STREAMS=2 (opt-in): odd chunks on a second compute stream.  With chunks of the size a rank of an 8-GPU job
        // transforms (32 x' of 1024: 12 short launches per apply) the ramp of a chunk's kernels fills the tail of the previous chunk's --
        // one rank, 32 such chunks at 512^3: 15.93 -> 15.25-15.5 ms; neutral with 4 or 8 large chunks (profiles/r03_dist_two_compute_streams.log).
        // Not the default: that was measured with device-to-device copies as the exchange; RCCL's transfer kernels need CUs, which
        // they get at the boundaries between compute kernels -- two compute streams close those gaps, and no multi-GPU node has
        // been available to see what that does to the exchange.
        const char* cse = getenv("LSFC_DIST_COMPUTE_STREAMS");
        if (K >= 2 && cse && atoi(cse) == 2) LSFC_HIP(hipStreamCreateWithFlags(&d->st2, hipStreamNonBlocking));
        for (hipEvent_t* e : { &d->ev_p1, &d->ev_p1a, &d->ev_backa }) LSFC_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
        d->ev_in.resize((size_t)K); d->ev_done.resize((size_t)K); d->ev_back.resize((size_t)K);
        for (int c = 0; c < K; ++c) {
            LSFC_HIP(hipEventCreateWithFlags(&d->ev_in[c], hipEventDisableTiming));
            LSFC_HIP(hipEventCreateWithFlags(&d->ev_done[c], hipEventDisableTiming));
            LSFC_HIP(hipEventCreateWithFlags(&d->ev_back[c], hipEventDisableTiming));
        }
    }
    // symbol: every rank evaluates the reduced symbol (elementary functions + rocFFT; 0.2 s at 512^3 through the symbol's
    // symmetry, 8.6 GB of temporaries that are freed before the message buffers and A2 are allocated) and keeps
    // only the slab of its own x' tiles in the tiled storage order
    DevBuf<cplx> G2;
    const bool quarter = plan_quarter_symbol_ok(p.get());
    if (quarter) symbol_gv3d_quarter(p.get(), box, G2); else symbol_gv3d_reduced(p.get(), box, G2);
    std::vector<int> perm[3]; DevBuf<int> dperm[3];
    for (int a = 0; a < 3; ++a) {
        perm[a].resize((size_t)p->pads[a]);
        pruned_perm(p->pads[a], perm[a].data());
        dperm[a].alloc(perm[a].size());
        LSFC_HIP(hipMemcpy(dperm[a].p, perm[a].data(), perm[a].size() * sizeof(int), hipMemcpyHostToDevice));
        plan_make_twiddles(p.get(), a, p->pads[a]);
    }
    const int ntiles = d->W / 8;
    const double scale = 1.0 / ((double)p->pads[0] * p->pads[1] * p->pads[2]);
    DevBuf<int> pyrow;
    plan_setup_symbol_rows(p.get(), quarter ? nullptr : G2.p, perm[1], perm[2], pyrow);
    p->sym.alloc((size_t)d->W * p->sym_rows * p->sym_hz);
    pw_permute_symbol(G2.p, p->sym.p, dperm[0].p, pyrow.p, dperm[2].p, p->pads, p->sym_rows, p->sym_hz, rank * ntiles, ntiles, scale, p->stream,
                      quarter ? p->pads[1] / 2 + 1 : 0);
    LSFC_HIP(hipStreamSynchronize(p->stream));
    G2.release();
    d->S1.alloc((size_t)p->pads[0] * m * lz);
    d->R1.alloc((size_t)d->W * m * l);
    // A2 rows are padded like the single-GPU plan's (the message buffers S1 / R1 stay dense: their blocks are the messages)
    const int pad2 = p->tuning.pad2 >= 0 ? p->tuning.pad2 : (p->pads[1] >= 1024 ? 72 : 0);
    p->pitch1 = d->Wc;
    p->pitch2 = 8 * (int)l + pad2 / 8 * 8;
    p->A2.alloc((size_t)(d->W / 8) * p->pads[1] * p->pitch2);
    LSFC_HIP(hipMemset(d->S1.p, 0, d->S1.bytes()));
    LSFC_HIP(hipMemset(d->R1.p, 0, d->R1.bytes()));
    LSFC_HIP(hipMemset(p->A2.p, 0, p->A2.bytes()));
    p->pipeline = lsfc_plan::PRUNED;
    *out = p.release();
}


// ---------------------------------------------------------------------------
// Single-process multi-device plan: ONE host thread enqueues the work of all P ranks (one per device).  The schedule
// is the one dist_convolve_dev runs (pipelined_convolve), with all P ranks local: a wait "of every rank" then covers them
// all (a stream of one device may wait on an event of another).  Two transports for the slab exchanges:
//   rccl  grouped ncclSend/ncclRecv over the communicators of ncclCommInitAll (distinct devices; the default)
//   copy  hipMemcpyPeerAsync issued by the SOURCE rank on its communication stream (copy engines instead of CUs; also
//         the only form that runs with a device listed twice, which is how the driver is tested on a one-GPU box)
// ---------------------------------------------------------------------------
MultiState::~MultiState() {
    for (void* c : comm2) if (c) (void)ncclCommDestroy((ncclComm_t)c);
    for (void* c : comm) if (c) (void)ncclCommDestroy((ncclComm_t)c);
    if (red_pin) (void)hipHostFree(red_pin);
}

void multi_synchronize(lsfc_plan* root) {
    Local(root).each([](int) { LSFC_HIP(hipDeviceSynchronize()); });
}

void multi_convolve_dev(lsfc_plan* root, const cplx* const* x, cplx* const* y, const ConvOp& op) {
    LSFC_REQUIRE(conv_forward_only(op), "the transposed and the adjoint operator are not available on a multi-device plan");
    const Local L(root);
    // LSFC_DIST_OVERLAP=0: the same steps, no split of the pipeline ends, the host between the passes of a chunk and its way back
    const bool overlap = !L.d(0)->no_overlap;
    pipelined_convolve(L, x, y, op, overlap && L.d(0)->split_edges && L.d(0)->lz % 2 == 0, !overlap);
}

// ---------------------------------------------------------------------------
// A team of slabs (team.hpp)
SlabTeam::SlabTeam(lsfc_plan* r) : root(r), multi(r->multi != nullptr) {
    if (!multi) { slabs.push_back({r, r->device, 0, r->N, 0}); return; }
    int64_t off = 0;
    for (auto& sp : r->multi->sub) { slabs.push_back({sp.get(), sp->device, (int)slabs.size(), sp->N, off}); off += sp->N; }
}
void SlabTeam::apply(const cplx* const* in, cplx* const* out) const {
    if (multi) multi_convolve_dev(root, in, out, plan_operator(root));
    else plan_apply_dev(root, in[0], out[0]);
}
void SlabTeam::scatter(const cplx* x, const cplx* b) const {
    each([&](const RankSlab& s) {
        plan_ensure_staging(s.p, s.n);
        LSFC_HIP(hipMemcpyAsync(s.p->xs.p, x + s.off, (size_t)s.n * sizeof(cplx), hipMemcpyHostToDevice, s.st()));
        if (b) LSFC_HIP(hipMemcpyAsync(s.p->ys.p, b + s.off, (size_t)s.n * sizeof(cplx), hipMemcpyHostToDevice, s.st()));
    });
}
void SlabTeam::gather(cplx* x, bool from_ys) const {
    each([&](const RankSlab& s) { LSFC_HIP(hipMemcpyAsync(x + s.off, from_ys ? s.p->ys.p : s.p->xs.p, (size_t)s.n * sizeof(cplx), hipMemcpyDeviceToHost, s.st())); });
}

void multi_convolve_host(lsfc_plan* root, const cplx* x, cplx* y, const ConvOp& op) {
    LSFC_REQUIRE(conv_forward_only(op), "the transposed and the adjoint operator are not available on a multi-device plan");
    const SlabTeam T(root);
    T.scatter(x, nullptr);
    std::vector<const cplx*> xd; std::vector<cplx*> yd;
    for (const RankSlab& s : T.slabs) { xd.push_back(s.p->xs.p); yd.push_back(s.p->ys.p); }
    multi_convolve_dev(root, xd.data(), yd.data(), op);
    T.gather(y, true);
    T.sync();
}

// sum over the ranks of `count` complex scalars held at dev[r] on devices[r]; the result replaces every copy
void multi_allreduce_sum(lsfc_plan* root, cplx* const* dev, int count) {
    const Local L(root);
    MultiState* ms = root->multi.get();
    const int P = L.P;
    auto st = [&](int r) { return L.stream(r, Lane::COMPUTE); };
    if (P == 1) return;
    if (ms->rccl) {
        LSFC_NCCL(ncclGroupStart());
        for (int r = 0; r < P; ++r)
            LSFC_NCCL(ncclAllReduce(dev[r], dev[r], (size_t)count * 2, ncclDouble, ncclSum, (ncclComm_t)ms->comm[(size_t)r], st(r)));
        LSFC_NCCL(ncclGroupEnd());
        return;
    }
    // copy transport: O(restart) scalars through pinned host memory, summed in rank order (reproducible); the pinned scratch
    // holds 256 scalars per rank, longer reductions (classical Gram-Schmidt with restart > 256) go in pieces
    if (count > 256) {
        for (int c0 = 0; c0 < count; c0 += 256) {
            std::vector<cplx*> piece((size_t)P);
            for (int r = 0; r < P; ++r) piece[(size_t)r] = dev[r] + c0;
            multi_allreduce_sum(root, piece.data(), std::min(256, count - c0));
        }
        return;
    }
    cplx* pin = ms->red_pin;
    L.each([&](int r) { LSFC_HIP(hipMemcpyAsync(pin + (size_t)(r + 1) * 256, dev[r], (size_t)count * sizeof(cplx), hipMemcpyDeviceToHost, st(r))); });
    L.each([&](int r) { LSFC_HIP(hipStreamSynchronize(st(r))); });
    for (int i = 0; i < count; ++i) {
        cplx acc = make_double2(0.0, 0.0);
        for (int r = 0; r < P; ++r) { acc.x += pin[(size_t)(r + 1) * 256 + i].x; acc.y += pin[(size_t)(r + 1) * 256 + i].y; }
        pin[i] = acc;
    }
    L.each([&](int r) { LSFC_HIP(hipMemcpyAsync(dev[r], pin, (size_t)count * sizeof(cplx), hipMemcpyHostToDevice, st(r))); });
    // (the next reduction rewrites the pinned scratch: it starts with copies INTO it that are stream-ordered behind these, and the
    // host only touches it after synchronising every rank's stream above)
}

// per-stage timing of one apply on the ranks' staging vectors: every stage runs on all ranks, un-overlapped, with a
// device-wide synchronisation in between; the time of a stage is the slowest rank's
void multi_profile(lsfc_plan* root, int reps, int max_stages, const char** names, double* ms, double* bytes, int* nstages) {
    const Local L(root);
    const int P = L.P;
    std::vector<const cplx*> xd; std::vector<cplx*> yd;
    L.each([&](int r) {
        lsfc_plan* p = L.plan[(size_t)r];
        const bool fresh = p->xs.n < (size_t)p->N;
        plan_ensure_staging(p, p->N);
        if (fresh) LSFC_HIP(hipMemset(p->xs.p, 0, p->xs.bytes()));
        xd.push_back(p->xs.p); yd.push_back(p->ys.p);
    });
    const std::vector<Stage> stages = apply_stages(L, xd, yd, true);
    LSFC_REQUIRE((int)stages.size() <= max_stages, "max_stages too small (need %d)", (int)stages.size());
    *nstages = (int)stages.size();
    std::vector<hipEvent_t> e0((size_t)P), e1((size_t)P);
    L.each([&](int r) { LSFC_HIP(hipEventCreate(&e0[(size_t)r])); LSFC_HIP(hipEventCreate(&e1[(size_t)r])); });
    for (size_t i = 0; i < stages.size(); ++i) { names[i] = stages[i].name; bytes[i] = stages[i].bytes; ms[i] = 0.0; }
    for (int rep = 0; rep < reps; ++rep)
        for (size_t i = 0; i < stages.size(); ++i) {
            multi_synchronize(root);
            L.each([&](int r) { LSFC_HIP(hipEventRecord(e0[(size_t)r], L.stream(r, Lane::COMPUTE))); });
            stages[i].run();
            L.each([&](int r) { LSFC_HIP(hipEventRecord(e1[(size_t)r], L.stream(r, Lane::COMPUTE))); });
            multi_synchronize(root);
            float worst = 0;
            for (int r = 0; r < P; ++r) { float t = 0; LSFC_HIP(hipEventElapsedTime(&t, e0[(size_t)r], e1[(size_t)r])); worst = std::max(worst, t); }
            ms[i] += worst;
        }
    for (size_t i = 0; i < stages.size(); ++i) ms[i] /= reps;
    for (int r = 0; r < P; ++r) { (void)hipEventDestroy(e0[(size_t)r]); (void)hipEventDestroy(e1[(size_t)r]); }
}

static void create_multi_plan(lsfc_plan** out, int64_t n, int64_t m, int64_t l, double box, double omega, const double* nu,
                              unsigned flags, const int* devices, int ndev) {
    LSFC_REQUIRE(out, "NULL argument"); *out = nullptr;
    LSFC_REQUIRE(devices && ndev >= 1 && ndev <= 64, "devices[] / ndev: need 1..64 devices");
    LSFC_REQUIRE(nu, "nu is NULL");
    LSFC_REQUIRE(l % ndev == 0, "l = %lld is not divisible by the number of devices %d", (long long)l, ndev);
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) fail(LSFC_ENODEV, "no HIP device available: the lsfc operator has no CPU fallback");
    bool distinct = true;
    for (int r = 0; r < ndev; ++r) {
        LSFC_REQUIRE(devices[r] >= 0 && devices[r] < count, "device %d out of range (have %d)", devices[r], count);
        for (int q = 0; q < r; ++q) if (devices[q] == devices[r]) distinct = false;
    }
    std::unique_ptr<lsfc_plan> root(new lsfc_plan());
    root->device = devices[0]; root->ndim = 3;
    root->dims[0] = (int)n; root->dims[1] = (int)m; root->dims[2] = (int)l;
    root->N = n * m * l; root->omega = omega; root->quad_rule = LSFC_QUAD_GREENGARD_VICO; root->flags = flags;
    root->pipeline = lsfc_plan::PRUNED;
    root->multi.reset(new MultiState());
    MultiState* ms = root->multi.get();
    ms->P = ndev; ms->devices.assign(devices, devices + ndev);
    // transport: RCCL whenever the devices are distinct (LSFC_MULTI_TRANSPORT=copy selects the copy engines instead);
    // a device listed more than once (tests on a one-GPU box) can only use copies
    const char* tr = getenv("LSFC_MULTI_TRANSPORT");
    ms->rccl = distinct && !(tr && std::string(tr) == "copy");
    LSFC_REQUIRE(distinct || !(tr && std::string(tr) == "rccl"), "LSFC_MULTI_TRANSPORT=rccl needs distinct devices");
    // the ranks are built concurrently, one helper thread per device (symbol evaluation + rocFFT plan compilation are
    // the long part); ranks that share a device are built one after the other
    const int64_t nloc = n * m * (l / ndev);
    ms->sub.resize((size_t)ndev);
    std::vector<int> rc((size_t)ndev, LSFC_OK); std::vector<std::string> msg((size_t)ndev);
    auto build = [&](int r) {
        lsfc_plan* sp = nullptr;
        rc[(size_t)r] = guarded([&] { create_dist_plan(&sp, n, m, l, box, omega, nu + (int64_t)r * nloc, flags, devices[r], r, ndev, nullptr, false, true); });
        if (rc[(size_t)r] != LSFC_OK) msg[(size_t)r] = lsfc_last_error();
        ms->sub[(size_t)r].reset(sp);
    };
    if (distinct && ndev > 1) {
        std::vector<std::thread> th;
        for (int r = 0; r < ndev; ++r) th.emplace_back(build, r);
        for (auto& t : th) t.join();
    } else for (int r = 0; r < ndev; ++r) build(r);
    for (int r = 0; r < ndev; ++r) if (rc[(size_t)r] != LSFC_OK) fail(rc[(size_t)r], "rank %d on device %d: %s", r, devices[r], msg[(size_t)r].c_str());
    for (int d = 0; d < 3; ++d) root->pads[d] = ms->sub[0]->pads[d];
    if (distinct && ndev > 1) {
        // peer access for the copy transport (and for RCCL's own P2P paths)
        for (int r = 0; r < ndev; ++r) {
            LSFC_HIP(hipSetDevice(devices[r]));
            for (int q = 0; q < ndev; ++q) if (q != r) {
                int can = 0; LSFC_HIP(hipDeviceCanAccessPeer(&can, devices[r], devices[q]));
                if (can) { hipError_t pe = hipDeviceEnablePeerAccess(devices[q], 0); if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) LSFC_HIP(pe); (void)hipGetLastError(); }
                else LSFC_REQUIRE(ms->rccl, "device %d cannot access device %d: the copy transport needs peer access", devices[r], devices[q]);
            }
        }
    }
    if (ms->rccl && ndev > 1) {
        std::vector<ncclComm_t> c1((size_t)ndev), c2((size_t)ndev);
        LSFC_NCCL(ncclCommInitAll(c1.data(), ndev, devices));
        ms->comm.assign(c1.begin(), c1.end());
        LSFC_NCCL(ncclCommInitAll(c2.data(), ndev, devices));
        ms->comm2.assign(c2.begin(), c2.end());
    } else ms->rccl = ms->rccl && ndev > 1;
    LSFC_HIP(hipSetDevice(devices[0]));
    LSFC_HIP(hipHostMalloc((void**)&ms->red_pin, (size_t)(ndev + 1) * 256 * sizeof(cplx)));
    *out = root.release();
}

} // namespace lsfc

using namespace lsfc;

extern "C" {

int lsfc_plan_create_gv3d_multi(lsfc_plan** out, int64_t n, int64_t m, int64_t l, double box, double omega, const double* nu,
                                unsigned flags, const int* devices, int ndev) {
    return guarded([&] { create_multi_plan(out, n, m, l, box, omega, nu, flags, devices, ndev); });
}

int lsfc_multi_info(const lsfc_plan* plan, int* ndev, int* devices, int64_t* local_n, const char** transport) {
    return guarded([&] {
        LSFC_REQUIRE(plan && plan->multi, "not a multi-device plan");
        const MultiState* ms = plan->multi.get();
        if (ndev) *ndev = ms->P;
        if (devices) for (int r = 0; r < ms->P; ++r) devices[r] = ms->devices[(size_t)r];
        if (local_n) *local_n = ms->sub[0]->N;
        if (transport) *transport = ms->P == 1 ? "none (one device)" : (ms->rccl ? "rccl send/recv (ncclCommInitAll), pairwise schedule" : "peer copies (hipMemcpyPeerAsync), source-issued");
    });
}

int lsfc_multi_apply_dev(lsfc_plan* plan, const double* const* x_dev, double* const* y_dev, int mode) {
    return guarded([&] {
        LSFC_REQUIRE(plan && plan->multi && x_dev && y_dev, "not a multi-device plan / NULL argument");
        LSFC_REQUIRE(mode >= 0 && mode <= 2, "mode must be 0 (apply), 1 (convolve) or 2 (convolve with nu)");
        multi_convolve_dev(plan, (const cplx* const*)x_dev, (cplx* const*)y_dev, mode == 0 ? plan_operator(plan) : conv_plain(mode == 2, 0.0, 1.0));
    });
}

int lsfc_dist_unique_id(unsigned char id[LSFC_UNIQUE_ID_BYTES]) {
    return guarded([&] {
        LSFC_REQUIRE(id, "NULL argument");
        ncclUniqueId uid;
        LSFC_NCCL(ncclGetUniqueId(&uid));
        memcpy(id, &uid, LSFC_UNIQUE_ID_BYTES);
    });
}

int lsfc_dist_plan_create_gv3d(lsfc_plan** out, int64_t n, int64_t m, int64_t l, double box, double omega, const double* nu_local,
                               unsigned flags, int device, int rank, int nranks, const unsigned char id[LSFC_UNIQUE_ID_BYTES]) {
    return guarded([&] { create_dist_plan(out, n, m, l, box, omega, nu_local, flags, device, rank, nranks, id, false); });
}

int lsfc_dist_sim_plan_create_gv3d(lsfc_plan** out, int64_t n, int64_t m, int64_t l, double box, double omega, const double* nu_local,
                                   unsigned flags, int device, int rank, int nranks) {
    return guarded([&] { create_dist_plan(out, n, m, l, box, omega, nu_local, flags, device, rank, nranks, nullptr, true); });
}

int lsfc_dist_sim_apply(lsfc_plan** plans, int nranks, const double* const* x, double* const* y, int mode) {
    return guarded([&] {
        LSFC_REQUIRE(plans && x && y && nranks >= 1, "bad argument");
        for (int r = 0; r < nranks; ++r)
            LSFC_REQUIRE(plans[r] && plans[r]->dist && plans[r]->dist->sim && plans[r]->dist->nranks == nranks && plans[r]->dist->rank == r,
                         "plan %d is not simulated rank %d of %d", r, r, nranks);
        LSFC_REQUIRE(mode >= 0 && mode <= 2, "mode must be 0 (apply), 1 (convolve) or 2 (convolve with nu)");
        LSFC_HIP(hipSetDevice(plans[0]->device));
        const int64_t B = block_elems(plans[0]);
        auto sync_all = [&] { for (int r = 0; r < nranks; ++r) LSFC_HIP(hipStreamSynchronize(plans[r]->stream)); };
        // host vectors: stage through each plan's staging buffers
        std::vector<const cplx*> xd((size_t)nranks); std::vector<cplx*> yd((size_t)nranks);
        for (int r = 0; r < nranks; ++r) {
            lsfc_plan* p = plans[r];
            plan_ensure_staging(p, p->N);
            LSFC_HIP(hipMemcpy(p->xs.p, x[r], (size_t)p->N * sizeof(cplx), hipMemcpyHostToDevice));
            xd[r] = p->xs.p; yd[r] = p->ys.p;
        }
        const int K = plans[0]->dist->K;
        for (int r = 0; r < nranks; ++r) phase1(plans[r], xd[r], mode != 1, plans[r]->stream);
        sync_all();
        for (int c = 0; c < K; ++c) {
            // way in: block (q*K + c) of rank r's S1 -> slot r of chunk c of rank q's R1
            for (int r = 0; r < nranks; ++r) for (int q = 0; q < nranks; ++q)
                LSFC_HIP(hipMemcpy(plans[q]->dist->R1.p + dsched::r1_slot(c, nranks, r, B), plans[r]->dist->S1.p + dsched::s1_block(q, K, c, B),
                                   (size_t)B * sizeof(cplx), hipMemcpyDeviceToDevice));
            for (int r = 0; r < nranks; ++r) phase2(plans[r], c, plans[r]->stream);
            sync_all();
            // way back: slot q of chunk c of rank r's R1 -> block (r*K + c) of rank q's S1
            for (int r = 0; r < nranks; ++r) for (int q = 0; q < nranks; ++q)
                LSFC_HIP(hipMemcpy(plans[q]->dist->S1.p + dsched::s1_block(r, K, c, B), plans[r]->dist->R1.p + dsched::r1_slot(c, nranks, q, B),
                                   (size_t)B * sizeof(cplx), hipMemcpyDeviceToDevice));
        }
        for (int r = 0; r < nranks; ++r) {
            lsfc_plan* p = plans[r];
            if (mode == 0) phase3(p, xd[r], yd[r], 1.0, p->omega * p->omega, p->stream); else phase3(p, xd[r], yd[r], 0.0, 1.0, p->stream);
        }
        sync_all();
        for (int r = 0; r < nranks; ++r) LSFC_HIP(hipMemcpy(y[r], yd[r], (size_t)plans[r]->N * sizeof(cplx), hipMemcpyDeviceToHost));
    });
}

} // extern "C"
