// Host arithmetic of the slab-distributed apply (dist.hip): how the owned x' range is cut into pipeline chunks, where the
// block of a (rank, chunk) pair sits in the message buffers, and which messages a rank posts -- in which order -- for one
// exchange.  Pure C++ (no HIP, no RCCL): dist.hip issues exactly this list through ncclSend / ncclRecv (or peer copies),
// tests/emu/dist_schedule_test.cpp checks it for P = 2, 4, 8 ranks without a GPU, and tests/test_distributed_cpu.py drives
// it over real gloo ranks.
//
// Buffers of rank r (complex elements; B = Wc * m * lz = one block):
//   S1 [P][K][B]  block (q, c) = what the x pass wrote for destination rank q, chunk c (way in: sent to q)
//                               = what came back from source rank q, chunk c          (way back: received from q)
//   R1 [K][P][B]  slot (c, q)  = block received from source rank q for chunk c        (way in)
//                               = z range of rank q of the transformed chunk c         (way back: sent to q)
// A block is [z][m][Wc] with z slowest, so its two z halves are its two contiguous halves (part 0 / 1).
#pragma once
#include <cstdint>
#include <vector>

namespace lsfc { namespace dsched {

struct Chunks { int W, K, Wc; };
// W = Lx / P storage indices of x' per rank; K <= requested chunks of at least one 8-wide tile each, K | W
inline Chunks plan_chunks(int Lx, int nranks, int requested) {
    Chunks ch; ch.W = Lx / nranks;
    int K = requested < 1 ? 1 : requested;
    while (K > 1 && (ch.W % K != 0 || (ch.W / K) % 8 != 0)) --K;
    ch.K = K; ch.Wc = ch.W / K;
    return ch;
}
inline int64_t s1_block(int q, int K, int c, int64_t B) { return ((int64_t)q * K + c) * B; }
inline int64_t r1_slot(int c, int P, int q, int64_t B) { return ((int64_t)c * P + q) * B; }

struct Msg {
    int peer;          // the other rank (== own rank: the local copy)
    bool send;         // send (read the buffer) or receive (write it)
    bool in_s1;        // the buffer: S1 or R1
    int64_t off, count;   // complex elements
};
// Messages of exchange (c, back, part) as rank `rank` posts them inside one group: first the local copy (as a send / receive
// pair with peer == rank), then for s = 1 .. P - 1 a send to rank + s and a receive from rank - s (pairwise schedule: in step s
// every rank talks to a different peer, so all links of a fully connected node carry traffic at once).
inline std::vector<Msg> exchange_messages(int rank, int P, int K, int c, bool back, int part, int64_t Bfull) {
    const int64_t B = part < 0 ? Bfull : Bfull / 2, off = part == 1 ? Bfull / 2 : 0;
    std::vector<Msg> out;
    auto s1 = [&](int q) { return s1_block(q, K, c, Bfull) + off; };
    auto r1 = [&](int q) { return r1_slot(c, P, q, Bfull) + off; };
    // way in: S1 block (q, c) -> rank q, lands in R1 slot (c, <source>); way back: R1 slot (c, q) -> rank q, lands in S1 block (<source>, c)
    out.push_back(Msg{rank, true, !back, back ? r1(rank) : s1(rank), B});
    out.push_back(Msg{rank, false, back, back ? s1(rank) : r1(rank), B});
    for (int s = 1; s < P; ++s) {
        const int to = (rank + s) % P, from = (rank - s + P) % P;
        out.push_back(Msg{to, true, !back, back ? r1(to) : s1(to), B});
        out.push_back(Msg{from, false, back, back ? s1(from) : r1(from), B});
    }
    return out;
}

// ---------------------------------------------------------------------------
// The overlapped apply as data: the steps of one apply for one rank, in the order they are enqueued.  Streams of a rank:
// its compute stream, a second compute stream for the odd chunks (two_streams), one communication stream per direction.
// The x pass runs in two z halves where `edges` (part 0 / 1, else -1: whole), so that the first exchange starts after half of it;
// the way in of all chunks goes on IN; the y / z / y passes of chunk c run on the compute stream of its parity while the way back
// of chunk c - 1 goes on BACK; the last exchange back is split the same way and hides half of the inverse x pass.
// An event belongs to a rank.  A wait with `all` waits for that event of EVERY rank the process drives (one rank of a
// multi-process job, where RCCL orders the remote side; all P of a multi-device plan, where a block has landed once its
// source's event has fired); the others wait for the rank's own event.  BACK runs in order, so the event of the last
// exchange back covers the earlier chunks.
enum class Op { XFWD, EXCH_IN, PASSES, EXCH_BACK, XINV };
enum class Lane { COMPUTE, COMPUTE2, IN, BACK };
enum class Ev { NONE, P1A, P1, IN, DONE, BACKA, BACK };     // IN, DONE, BACK: one per chunk
struct Wait { Ev ev; int c; bool all; };
struct Step {
    Op op; int c, part;             // chunk (exchanges, passes) and z half (x passes, exchanges; -1: whole)
    Lane on;
    std::vector<Wait> waits;
    Ev rec; int rec_c;              // recorded behind the step (NONE: nothing)
};
inline bool is_exchange(Op op) { return op == Op::EXCH_IN || op == Op::EXCH_BACK; }

inline std::vector<Step> pipeline_steps(int K, bool edges, bool two_streams) {
    std::vector<Step> s;
    if (edges) s.push_back({Op::XFWD, 0, 0, Lane::COMPUTE, {}, Ev::P1A, 0});
    s.push_back({Op::XFWD, 0, edges ? 1 : -1, Lane::COMPUTE, {}, Ev::P1, 0});
    // way in.  A block may only land on a rank once that rank's previous apply has drained (its R1 / S1 are re-used): the x pass
    // of EVERY rank, which on each rank follows the previous apply's last pass
    if (edges) s.push_back({Op::EXCH_IN, 0, 0, Lane::IN, {{Ev::P1A, 0, true}}, Ev::NONE, 0});
    for (int c = 0; c < K; ++c) {
        std::vector<Wait> w;
        if (c == 0) w.push_back({Ev::P1, 0, true});
        s.push_back({Op::EXCH_IN, c, (edges && c == 0) ? 1 : -1, Lane::IN, w, Ev::IN, c});
    }
    for (int c = 0; c < K; ++c) {
        // (a chunk always runs on the stream of its parity, so its buffers -- A2 / R1 chunk c -- stay ordered from one apply to the next)
        s.push_back({Op::PASSES, c, -1, ((c & 1) && two_streams) ? Lane::COMPUTE2 : Lane::COMPUTE, {{Ev::IN, c, true}}, Ev::DONE, c});
        // (the S1 blocks the way back overwrites belong to chunk c, whose way in finished before IN[c]; P1: behind the previous
        // apply's inverse x pass, which read them)
        std::vector<Wait> w;
        if (c == 0) w.push_back({Ev::P1, 0, true});
        w.push_back({Ev::DONE, c, false});
        if (edges && c == K - 1) {
            s.push_back({Op::EXCH_BACK, c, 0, Lane::BACK, w, Ev::BACKA, 0});
            s.push_back({Op::EXCH_BACK, c, 1, Lane::BACK, {}, Ev::BACK, c});
        } else s.push_back({Op::EXCH_BACK, c, -1, Lane::BACK, w, Ev::BACK, c});
    }
    if (edges) s.push_back({Op::XINV, 0, 0, Lane::COMPUTE, {{Ev::BACKA, 0, true}}, Ev::NONE, 0});
    s.push_back({Op::XINV, 0, edges ? 1 : -1, Lane::COMPUTE, {{Ev::BACK, K - 1, true}}, Ev::NONE, 0});
    return s;
}

// Enqueues the steps for the nlocal ranks a process drives, step by step: the waits of every rank, the step itself -- an
// exchange once for all ranks (one RCCL group, or source-issued copies), anything else rank by rank -- and the records.
// Every record of a step is enqueued before any wait of a later one, which is what lets a stream wait for another rank's event.
// Sink: begin(step), wait(r, lane, q, ev, c), run(r, step), exchange(step), record(r, lane, ev, c).
template <class Sink> void issue(const std::vector<Step>& steps, int nlocal, Sink& sink) {
    for (const Step& s : steps) {
        sink.begin(s);
        for (int r = 0; r < nlocal; ++r) {
            for (const Wait& w : s.waits)
                for (int q = w.all ? 0 : r; q < (w.all ? nlocal : r + 1); ++q) sink.wait(r, s.on, q, w.ev, w.c);
            if (is_exchange(s.op)) continue;
            sink.run(r, s);
            if (s.rec != Ev::NONE) sink.record(r, s.on, s.rec, s.rec_c);
        }
        if (!is_exchange(s.op)) continue;
        sink.exchange(s);
        if (s.rec != Ev::NONE) for (int r = 0; r < nlocal; ++r) sink.record(r, s.on, s.rec, s.rec_c);
    }
}

}} // namespace lsfc::dsched
