// Running a plan on HOST vectors: the chunked upload / transform / download pipeline for large 3D vectors, one staged copy each
// way for the others, scatter and gather over the ranks of a multi-device plan (gfx950).
#include "plan.hpp"
#include "apply.hpp"
#include <condition_variable>
#include <deque>
#include <mutex>
#include <optional>
#include <thread>

namespace lsfc {

void plan_ensure_staging(lsfc_plan* p, int64_t count) {
    if (p->xs.n < (size_t)count) { p->xs.alloc((size_t)count); p->ys.alloc((size_t)count); }
}

HostPipe::~HostPipe() {
    for (hipEvent_t e : ev_up) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_down) (void)hipEventDestroy(e);
    if (ev_free) (void)hipEventDestroy(ev_free);
    for (hipEvent_t e : { ev_xfree[0], ev_xfree[1], ev_yfree[0], ev_yfree[1] }) if (e) (void)hipEventDestroy(e);
    if (up) (void)hipStreamDestroy(up);
    if (down) (void)hipStreamDestroy(down);
}

// The drop-in path the reference exercises, mul!(Y, M, b) with HOST vectors (src/FastConvolution.jl:50-54), as a pipeline over
// K chunks of z planes: chunk c of x travels host -> device on its own stream while the x and y passes of the chunks already
// landed run (those passes work plane by plane: yfwd of plane z needs xfwd of plane z only); then the fused z pass, which needs
// every plane; then the inverse y and x passes chunk by chunk, each chunk of y leaving for the host as soon as it exists.
// What cannot overlap: the first byte of y depends on the last byte of x (the Green's kernel is dense), so the upload and
// the download of ONE apply are strictly one after the other -- the floor is 2 N 16 B / PCIe rate + the fused pass
// (512^3: 2 x 37.5 ms at the 57 GB/s this box moves per direction + 4.7 ms), not the full-duplex rate.
// Caller memory: pageable vectors go through the runtime's staged copies (measured 56 / 50 GB/s up / down, no slower than
// pinned on this box); vectors registered with lsfc_host_register (or allocated pinned) are read and written by DMA directly.
static int host_pipeline_chunks(const lsfc_plan* p) {
    const char* e = getenv("LSFC_HOST_PIPELINE");                  // developer switch: 0 / 1 off, K >= 2 chunks whatever the size
    const int forced = e ? atoi(e) : -1;
    if (forced == 0 || forced == 1) return 1;
    if (p->pipeline != lsfc_plan::PRUNED || p->ndim != 3 || p->dist || p->multi) return 1;
    if (forced < 0 && p->N * (int64_t)sizeof(cplx) < ((int64_t)64 << 20)) return 1;       // small vectors: one copy each way
    const int l = p->dims[2];
    for (int K = forced > 1 ? forced : 8; K >= 2; --K) if (l % K == 0) return K;
    return 1;
}

// Several right-hand sides: the downloads are issued from a helper thread.  With pageable caller memory the runtime stages every
// copy through pinned buffers ON THE CALLING THREAD and returns when it is done, so downloads issued here would keep the
// uploads of the next right-hand side from even starting; from a second thread the two directions run side by side.
// The worker issues the queued downloads in order on the `down` stream.  finish() lets it issue what is queued and joins it;
// the destructor of a worker that was not finished (an exception on its way out) DISCARDS what is queued and joins it.
class DownloadWorker {
public:
    struct Job { hipEvent_t ev; cplx* dst; const cplx* src; int slot; bool last; int64_t rhs; };     // ev: the chunk at src is ready
    DownloadWorker(int device, HostPipe* hp, size_t chunk_bytes) : hp_(hp), bytes_(chunk_bytes), thread_([this, device] { run(device); }) {}
    DownloadWorker(const DownloadWorker&) = delete; DownloadWorker& operator=(const DownloadWorker&) = delete;
    ~DownloadWorker() { stop(true); }
    void push(const Job& j) { { std::lock_guard<std::mutex> lk(mu_); q_.push_back(j); } cv_.notify_all(); }
    // until the last download of right-hand side `rhs` out of staging slot `slot` has been issued and ev_yfree[slot] recorded behind it
    void wait_slot(int slot, int64_t rhs) {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return yfree_recorded_[slot] >= rhs + 1 || err_; });
        if (err_) std::rethrow_exception(err_);
    }
    void finish() { stop(false); if (err_) std::rethrow_exception(err_); }
private:
    void stop(bool discard) {
        if (!thread_.joinable()) return;
        { std::lock_guard<std::mutex> lk(mu_); done_ = true; if (discard) q_.clear(); }
        cv_.notify_all();
        thread_.join();
    }
    void run(int device) {
        try {
            LSFC_HIP(hipSetDevice(device));
            for (;;) {
                Job d;
                { std::unique_lock<std::mutex> lk(mu_); cv_.wait(lk, [&] { return !q_.empty() || done_; }); if (q_.empty()) return; d = q_.front(); q_.pop_front(); }
                LSFC_HIP(hipStreamWaitEvent(hp_->down, d.ev, 0));
                LSFC_HIP(hipMemcpyAsync(d.dst, d.src, bytes_, hipMemcpyDeviceToHost, hp_->down));
                if (d.last) {
                    LSFC_HIP(hipEventRecord(hp_->ev_yfree[d.slot], hp_->down));
                    { std::lock_guard<std::mutex> lk(mu_); yfree_recorded_[d.slot] = d.rhs + 1; }
                    cv_.notify_all();
                }
            }
        } catch (...) { { std::lock_guard<std::mutex> lk(mu_); err_ = std::current_exception(); } cv_.notify_all(); }
    }
    HostPipe* hp_; size_t bytes_;
    std::mutex mu_; std::condition_variable cv_; std::deque<Job> q_; bool done_ = false; std::exception_ptr err_;
    int64_t yfree_recorded_[2] = { 0, 0 };             // slot s: 1 + the last right-hand side whose final download has been issued (and ev_yfree recorded)
    std::thread thread_;                               // (last: it starts on the members above)
};

// nrhs right-hand sides through the pipeline with TWO staging slots: while right-hand side j is transformed back and its chunks leave
// for the host, the chunks of right-hand side j + 1 arrive -- across right-hand sides the two PCIe directions do overlap (512^3: 53-55
// ms per right-hand side against 83-87 for one alone).
static void host_pipelined_convolve(lsfc_plan* p, const cplx* x, cplx* y, int64_t nrhs, const ConvOp& op, int K) {
    if (!p->hostpipe) {
        std::unique_ptr<HostPipe> hp(new HostPipe());
        LSFC_HIP(hipStreamCreateWithFlags(&hp->up, hipStreamNonBlocking));
        LSFC_HIP(hipStreamCreateWithFlags(&hp->down, hipStreamNonBlocking));
        LSFC_HIP(hipEventCreateWithFlags(&hp->ev_free, hipEventDisableTiming));
        for (hipEvent_t* e : { &hp->ev_xfree[0], &hp->ev_xfree[1], &hp->ev_yfree[0], &hp->ev_yfree[1] }) LSFC_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
        p->hostpipe = std::move(hp);
    }
    HostPipe* hp = p->hostpipe.get();
    while ((int)hp->ev_up.size() < 2 * K) {
        hipEvent_t a, b;
        LSFC_HIP(hipEventCreateWithFlags(&a, hipEventDisableTiming)); hp->ev_up.push_back(a);
        LSFC_HIP(hipEventCreateWithFlags(&b, hipEventDisableTiming)); hp->ev_down.push_back(b);
    }
    const int slots = nrhs > 1 ? 2 : 1;
    if (p->xs.n < (size_t)(slots * p->N)) { LSFC_HIP(hipStreamSynchronize(p->stream)); plan_ensure_staging(p, slots * p->N); }
    hipStream_t st = p->stream;
    const int lz = p->dims[2] / K;
    const int64_t chunk = (int64_t)p->dims[0] * p->dims[1] * lz;
    std::optional<DownloadWorker> worker;              // (declared ahead of the try block: the handler below joins it first)
    try {
        // the staging buffers may still be read by work queued earlier on the plan's stream (device-memory calls are asynchronous)
        LSFC_HIP(hipEventRecord(hp->ev_free, st));
        LSFC_HIP(hipStreamWaitEvent(hp->up, hp->ev_free, 0));
        if (nrhs > 1) worker.emplace(p->device, hp, (size_t)chunk * sizeof(cplx));
        for (int64_t j = 0; j < nrhs; ++j) {
            const int sl = (int)(j % slots);
            const cplx* xj = x + j * p->N; cplx* yj = y + j * p->N;
            cplx* xs = p->xs.p + (int64_t)sl * p->N; cplx* ys = p->ys.p + (int64_t)sl * p->N;
            VecBatch sv{}; sv.x[0] = xs; sv.y[0] = ys;
            // slot sl was last used by right-hand side j - 2: its inverse x pass (which reads xs) and its downloads (which read ys) must be over
            if (j >= slots) {
                LSFC_HIP(hipStreamWaitEvent(hp->up, hp->ev_xfree[sl], 0));
                // (the event of the slot's last download is recorded by the worker: wait until it has been, then order the stream behind it)
                if (worker) worker->wait_slot(sl, j - slots);
                LSFC_HIP(hipStreamWaitEvent(st, hp->ev_yfree[sl], 0));
            }
            for (int c = 0; c < K; ++c) {
                const int64_t off = c * chunk;
                hipEvent_t ev = hp->ev_up[(size_t)(sl * K + c)];
                LSFC_HIP(hipMemcpyAsync(xs + off, xj + off, (size_t)chunk * sizeof(cplx), hipMemcpyHostToDevice, hp->up));
                LSFC_HIP(hipEventRecord(ev, hp->up));
                LSFC_HIP(hipStreamWaitEvent(st, ev, 0));
                pass_xfwd(p, sv, 1, op, Slab{c * lz, lz}, st);
                pass_yfwd(p, 1, Slab{c * lz, lz}, st);
            }
            pass_fused(p, 1, st);
            for (int c = 0; c < K; ++c) {
                const int64_t off = c * chunk;
                hipEvent_t ev = hp->ev_down[(size_t)(sl * K + c)];
                pass_yinv(p, 1, Slab{c * lz, lz}, st);
                pass_xinv(p, sv, 1, op, Slab{c * lz, lz}, st);
                LSFC_HIP(hipEventRecord(ev, st));
                if (worker) worker->push({ev, yj + off, ys + off, sl, c == K - 1, j});
                else {
                    LSFC_HIP(hipStreamWaitEvent(hp->down, ev, 0));
                    LSFC_HIP(hipMemcpyAsync(yj + off, ys + off, (size_t)chunk * sizeof(cplx), hipMemcpyDeviceToHost, hp->down));
                }
            }
            LSFC_HIP(hipEventRecord(hp->ev_xfree[sl], st));
            if (!worker) LSFC_HIP(hipEventRecord(hp->ev_yfree[sl], hp->down));
        }
        if (worker) worker->finish();
        LSFC_HIP(hipStreamSynchronize(hp->down));
        LSFC_HIP(hipStreamSynchronize(st));
    } catch (...) {
        // The unwind (an error above, or the worker's own): nothing of this call may still be in flight when the caller sees the
        // error -- its vectors are its own again, and the next call orders only `up` behind the plan's stream.  The worker drops
        // what it has not issued and is joined; then the three streams drain, whatever they report.
        worker.reset();
        for (hipStream_t s : { hp->up, hp->down, st }) (void)hipStreamSynchronize(s);
        (void)hipGetLastError();
        throw;
    }
}

void host_convolve(lsfc_plan* p, const cplx* x, cplx* y, int64_t nrhs, const ConvOp& op) {
    if (p->multi) {
        // one host process, several devices: the vector is scattered over the ranks' z-slabs, applied, gathered
        for (int64_t j = 0; j < nrhs; ++j) multi_convolve_host(p, x + j * p->N, y + j * p->N, op);
        return;
    }
    // large 3D vectors: the chunked pipeline above (two staging slots, allocated there)
    const int K = host_pipeline_chunks(p);
    if (K > 1) {
        // (y aliasing x: right-hand side j + 1 is uploaded while j is downloaded into the same memory -- distinct vectors, no hazard)
        host_pipelined_convolve(p, x, y, nrhs, op, K);
        return;
    }
    plan_ensure_staging(p, p->N * std::min<int64_t>(LSFC_MAX_BATCH, nrhs));
    // LSFC_HOST_COPY=sync (developer switch, diagnostics of the round-2 first-apply fault): the round-2 workaround, a
    // synchronous copy behind a drained stream, instead of the stream-ordered copy
    static const bool sync_copy = env_switch("LSFC_HOST_COPY") == 's';
    for_each_group(nrhs, x, y, p->N, [&](int64_t, int cnt, const VecBatch& host) {
        const size_t bytes = (size_t)cnt * p->N * sizeof(cplx);
        if (sync_copy) {
            LSFC_HIP(hipStreamSynchronize(p->stream));
            LSFC_HIP(hipMemcpy(p->xs.p, host.x[0], bytes, hipMemcpyHostToDevice));
        } else LSFC_HIP(hipMemcpyAsync(p->xs.p, host.x[0], bytes, hipMemcpyHostToDevice, p->stream));
        plan_convolve_batch_dev(p, cnt, vec_batch(p->xs.p, p->ys.p, p->N, cnt), op);
        LSFC_HIP(hipMemcpyAsync(host.y[0], p->ys.p, bytes, hipMemcpyDeviceToHost, p->stream));
        LSFC_HIP(hipStreamSynchronize(p->stream));
    });
}

} // namespace lsfc
