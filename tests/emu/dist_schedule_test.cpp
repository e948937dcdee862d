// CPU check of the slab-exchange schedule that dist.hip posts through RCCL (csrc/dist_schedule.hpp), for P = 2, 4, 8 ranks,
// K = 1, 2, 4 chunks, both directions and the z-half split: every send has exactly one matching receive of equal size at the
// peer, in the same position of the (rank pair)'s message order; no two messages of an exchange overlap in a buffer; over
// all chunks (and halves) the messages tile the buffers exactly; in every step of the pairwise schedule each rank talks to a
// different peer.  Also the extern "C" surface the gloo test drives (built as a shared object with -DLSFC_SCHED_SHARED).
//
// Second part: the stream and event schedule of the overlapped apply (pipeline_steps, enqueued by issue -- the list and the
// order dist.hip executes), for P = 1, 2, 4 local ranks, K = 1, 2, 4 chunks, the pipeline ends split or not, one and two
// compute streams, TWO APPLIES BACK TO BACK.  Every stream is an in-order queue; a wait is an edge from the record it waits
// for; a block has landed when the copy of its source rank has run (the copy transport).  Checked: every wait finds its record
// enqueued ahead of it and the graph has no cycle; at the granularity of S1 half blocks, R1 half slots and A2 chunks, any two
// accesses of which one writes are ordered by the graph the way they were enqueued (a read after the write that produced it,
// an overwrite after the previous apply's reads); and the write a read sees is the one the pipeline means (the x pass for the
// way in, the way in for the passes, the passes for the way back, the way back for the inverse x pass, of the same apply).
#include "../../fast_solver_lippmann_schwinger_amd/csrc/dist_schedule.hpp"
#include <algorithm>
#include <cstdio>
#include <map>
#include <set>
#include <tuple>
using namespace lsfc::dsched;

extern "C" {
int lsfc_sched_plan_chunks(int Lx, int nranks, int requested, int* W, int* K, int* Wc) {
    const Chunks c = plan_chunks(Lx, nranks, requested); *W = c.W; *K = c.K; *Wc = c.Wc; return 0;
}
// messages of exchange (c, back, part) on `rank`: peer / send / in_s1 / off / count per message; returns their number
int lsfc_sched_exchange(int rank, int P, int K, int c, int back, int part, int64_t Bfull, int cap, int* peer, int* send, int* in_s1, int64_t* off, int64_t* count) {
    const std::vector<Msg> m = exchange_messages(rank, P, K, c, back != 0, part, Bfull);
    if ((int)m.size() > cap) return -1;
    for (size_t i = 0; i < m.size(); ++i) { peer[i] = m[i].peer; send[i] = m[i].send; in_s1[i] = m[i].in_s1; off[i] = m[i].off; count[i] = m[i].count; }
    return (int)m.size();
}
}

#ifndef LSFC_SCHED_SHARED
static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++bad; if (bad < 20) { printf("FAIL: " __VA_ARGS__); printf("\n"); } } } while (0)

// ---- the pipeline schedule as a graph ----
struct Access { int node, order; bool write; int apply; Op op; };
struct Graph {
    struct Node { std::vector<int> pred; };
    struct PendingWait { int node, apply, q; Ev ev; int c; };
    int P, K, apply = 0, order = 0;
    std::vector<Node> nodes;
    std::map<int, int> last;                                              // stream -> its newest node
    std::map<std::tuple<int, int, int, int>, int> rec;                    // (apply, rank, event, chunk) -> the record
    std::vector<PendingWait> waits;
    std::map<std::tuple<int, int, int, int, int>, std::vector<Access>> use;   // (buffer, rank, a, b, half) -> accesses as enqueued
    enum { S1 = 0, R1 = 1, A2 = 2 };

    int push(int r, Lane on) {
        const int s = r * 4 + (int)on, id = (int)nodes.size();
        nodes.push_back({});
        if (last.count(s)) nodes.back().pred.push_back(last[s]);
        last[s] = id;
        return id;
    }
    void touch(int node, const Step& s, bool write, int buf, int r, int a, int b, int half) {
        use[{buf, r, a, b, half}].push_back({node, order++, write, apply, s.op});
    }
    // the sink of issue()
    void begin(const Step&) {}
    void wait(int r, Lane on, int q, Ev ev, int c) { waits.push_back({push(r, on), apply, q, ev, c}); }
    void record(int r, Lane on, Ev ev, int c) { rec[{apply, r, (int)ev, c}] = push(r, on); }
    void run(int r, const Step& s) {
        const int n = push(r, s.on);
        for (int h = 0; h < 2; ++h) {
            if (s.op != Op::PASSES && s.part >= 0 && s.part != h) continue;
            for (int q = 0; q < P; ++q) {
                if (s.op == Op::PASSES) touch(n, s, false, R1, r, s.c, q, h);
                else for (int c = 0; c < K; ++c) touch(n, s, s.op == Op::XFWD, S1, r, q, c, h);
            }
        }
        if (s.op != Op::PASSES) return;
        touch(n, s, true, A2, r, s.c, 0, 0); touch(n, s, false, A2, r, s.c, 0, 0);
        for (int h = 0; h < 2; ++h) for (int q = 0; q < P; ++q) touch(n, s, true, R1, r, s.c, q, h);
    }
    void exchange(const Step& s) {
        for (int r = 0; r < P; ++r) {                                     // the source's stream carries its blocks
            const int n = push(r, s.on);
            for (int h = 0; h < 2; ++h) {
                if (s.part >= 0 && s.part != h) continue;
                for (int q = 0; q < P; ++q) {
                    if (s.op == Op::EXCH_IN) { touch(n, s, false, S1, r, q, s.c, h); touch(n, s, true, R1, q, s.c, r, h); }
                    else { touch(n, s, false, R1, r, s.c, q, h); touch(n, s, true, S1, q, r, s.c, h); }
                }
            }
        }
    }
};

// failures of one configuration (0: the schedule is sound); what: printed with the first failures
static int check_pipeline(const std::vector<Step>& steps, int P, int K, const char* what, bool quiet) {
    int fails = 0;
    auto FAIL = [&](const char* msg, int a, int b) { if (!quiet && fails < 5) printf("FAIL: %s: %s (%d, %d)\n", what, msg, a, b); ++fails; };
    Graph g; g.P = P; g.K = K;
    for (g.apply = 0; g.apply < 2; ++g.apply) issue(steps, P, g);
    // a wait means the record of its own apply; the runtime gives it the newest one enqueued AHEAD of it
    for (const auto& w : g.waits) {
        auto it = g.rec.find({w.apply, w.q, (int)w.ev, w.c});
        if (it == g.rec.end()) { FAIL("a wait for an event that is never recorded", (int)w.ev, w.c); continue; }
        if (it->second > w.node) FAIL("a wait enqueued ahead of its record", w.node, it->second);
        g.nodes[(size_t)w.node].pred.push_back(it->second);
    }
    // no wait cycle: every node runs once its predecessors have (Kahn), and what reaches what, in that order
    const int n = (int)g.nodes.size(), words = (n + 63) / 64;
    std::vector<int> indeg((size_t)n, 0), topo;
    std::vector<std::vector<int>> succ((size_t)n);
    for (int v = 0; v < n; ++v) for (int u : g.nodes[(size_t)v].pred) { succ[(size_t)u].push_back(v); ++indeg[(size_t)v]; }
    for (int v = 0; v < n; ++v) if (!indeg[(size_t)v]) topo.push_back(v);
    for (size_t i = 0; i < topo.size(); ++i) for (int v : succ[(size_t)topo[i]]) if (!--indeg[(size_t)v]) topo.push_back(v);
    if ((int)topo.size() != n) { FAIL("wait cycle: nodes that never run", n - (int)topo.size(), n); return fails; }
    std::vector<std::vector<uint64_t>> reach((size_t)n, std::vector<uint64_t>((size_t)words, 0));
    for (int v : topo) for (int u : g.nodes[(size_t)v].pred) {
        for (int k = 0; k < words; ++k) reach[(size_t)v][(size_t)k] |= reach[(size_t)u][(size_t)k];
        reach[(size_t)v][(size_t)(u / 64)] |= (uint64_t)1 << (u % 64);
    }
    auto before = [&](int a, int b) { return a == b || ((reach[(size_t)b][(size_t)(a / 64)] >> (a % 64)) & 1); };
    auto producer = [](Op reader) { return reader == Op::EXCH_IN ? Op::XFWD : reader == Op::PASSES ? Op::EXCH_IN : reader == Op::EXCH_BACK ? Op::PASSES : Op::EXCH_BACK; };
    for (const auto& kv : g.use) {
        const int buf = std::get<0>(kv.first);
        const std::vector<Access>& acc = kv.second;
        for (size_t j = 0; j < acc.size(); ++j) {
            const Access* made = nullptr;
            for (size_t i = 0; i < j; ++i) {
                if (acc[i].write) made = &acc[i];
                if (!(acc[i].write || acc[j].write) || before(acc[i].node, acc[j].node)) continue;
                FAIL(!acc[i].write ? "an overwrite that does not wait for an earlier read" : acc[j].write ? "two writes in no order" : "a read that does not wait for an earlier write", buf, acc[j].apply);
            }
            if (acc[j].write) continue;
            const Op want = buf == Graph::A2 ? Op::PASSES : producer(acc[j].op);
            if (!made || made->apply != acc[j].apply || made->op != want) FAIL("a read sees the wrong write", buf, acc[j].apply);
        }
    }
    return fails;
}

int main() {
    long checked = 0;
    for (int P : {1, 2, 4, 8}) for (int Kreq : {1, 2, 4, 8}) for (int Lx : {64, 96, 160, 1024, 1280, 1536}) {
        if ((Lx / 8) % P) continue;
        const Chunks ch = plan_chunks(Lx, P, Kreq);
        CHECK(ch.W * P == Lx && ch.K >= 1 && ch.K <= Kreq && ch.Wc * ch.K == ch.W && (ch.Wc % 8 == 0 || ch.K == 1), "plan_chunks(%d, %d, %d)", Lx, P, Kreq);
        const int K = ch.K;
        const int64_t B = (int64_t)ch.Wc * 6 * 4;               // m = 6, lz = 4 (even: z halves)
        for (int back = 0; back < 2; ++back) {
            // coverage of the buffers over all chunks: way in reads all of S1 and writes all of R1; way back the reverse
            for (int halves = 0; halves < 2; ++halves) {
                std::vector<std::vector<char>> rd((size_t)P, std::vector<char>((size_t)(P * K * B), 0)), wr = rd;
                for (int c = 0; c < K; ++c) for (int part : (halves ? std::vector<int>{0, 1} : std::vector<int>{-1})) {
                    std::vector<std::vector<Msg>> all((size_t)P);
                    for (int r = 0; r < P; ++r) all[(size_t)r] = exchange_messages(r, P, K, c, back != 0, part, B);
                    for (int r = 0; r < P; ++r) {
                        const auto& m = all[(size_t)r];
                        CHECK((int)m.size() == 2 * P, "message count");
                        CHECK(m[0].peer == r && m[0].send && m[1].peer == r && !m[1].send, "local copy first");
                        // pairwise steps: message 2s is the send to r + s, 2s + 1 the receive from r - s
                        std::set<int> to, from;
                        for (int s = 1; s < P; ++s) {
                            CHECK(m[(size_t)(2 * s)].send && m[(size_t)(2 * s)].peer == (r + s) % P, "send of step %d", s);
                            CHECK(!m[(size_t)(2 * s + 1)].send && m[(size_t)(2 * s + 1)].peer == (r - s + P) % P, "recv of step %d", s);
                            to.insert(m[(size_t)(2 * s)].peer); from.insert(m[(size_t)(2 * s + 1)].peer);
                        }
                        CHECK((int)to.size() == P - 1 && (int)from.size() == P - 1 && !to.count(r) && !from.count(r), "every peer exactly once");
                        for (const Msg& x : m) {
                            CHECK(x.count == (halves ? B / 2 : B), "message size");
                            CHECK(x.send ? (x.in_s1 == !back) : (x.in_s1 == (back != 0)), "buffer of a message");
                            auto& mark = x.send ? rd[(size_t)r] : wr[(size_t)r];
                            for (int64_t i = x.off; i < x.off + x.count; ++i) { CHECK(i >= 0 && i < (int64_t)mark.size() && !mark[(size_t)i], "overlap / out of range"); if (i >= 0 && i < (int64_t)mark.size()) mark[(size_t)i] = 1; }
                            ++checked;
                        }
                    }
                    // matching: the i-th send r -> q pairs with the i-th receive of q from r (one each per exchange), equal size,
                    // and the data lands where the layout says: way in block (q, c) of r's S1 -> slot (c, r) of q's R1
                    for (int r = 0; r < P; ++r) for (int q = 0; q < P; ++q) {
                        std::vector<Msg> snd, rcv;
                        for (const Msg& x : all[(size_t)r]) if (x.send && x.peer == q) snd.push_back(x);
                        for (const Msg& x : all[(size_t)q]) if (!x.send && x.peer == r) rcv.push_back(x);
                        CHECK(snd.size() == 1 && rcv.size() == 1 && snd[0].count == rcv[0].count, "send %d -> %d unmatched", r, q);
                        if (snd.size() == 1 && rcv.size() == 1) {
                            const int64_t ho = part == 1 ? B / 2 : 0;
                            CHECK(snd[0].off == (back ? r1_slot(c, P, q, B) : s1_block(q, K, c, B)) + ho, "send offset");
                            CHECK(rcv[0].off == (back ? s1_block(r, K, c, B) : r1_slot(c, P, r, B)) + ho, "recv offset");
                        }
                    }
                    // step s of the pairwise schedule: the sends of all ranks go to P different peers (all links busy at once)
                    for (int s = 1; s < P; ++s) { std::set<int> dst; for (int r = 0; r < P; ++r) dst.insert(all[(size_t)r][(size_t)(2 * s)].peer); CHECK((int)dst.size() == P, "step %d: a peer is addressed twice", s); }
                }
                for (int r = 0; r < P; ++r) {
                    CHECK(std::count(rd[(size_t)r].begin(), rd[(size_t)r].end(), 1) == (long)rd[(size_t)r].size(), "reads do not cover the source buffer (P=%d K=%d back=%d halves=%d)", P, K, back, halves);
                    CHECK(std::count(wr[(size_t)r].begin(), wr[(size_t)r].end(), 1) == (long)wr[(size_t)r].size(), "writes do not cover the destination buffer (P=%d K=%d back=%d halves=%d)", P, K, back, halves);
                }
            }
        }
    }
    // the pipeline schedule; then five broken ones, which the check must refuse
    long configs = 0;
    for (int P : {1, 2, 4}) for (int K : {1, 2, 4}) for (int edges = 0; edges < 2; ++edges) for (int two = 0; two < 2; ++two) {
        char what[64]; snprintf(what, sizeof what, "pipeline P=%d K=%d edges=%d streams=%d", P, K, edges, 1 + two);
        bad += check_pipeline(pipeline_steps(K, edges != 0, two != 0), P, K, what, false);
        ++configs;
    }
    for (int mut = 0; mut < 5; ++mut) {
        std::vector<Step> s = pipeline_steps(2, true, true);
        for (Step& st : s) {
            if (mut == 0 && st.op == Op::PASSES) st.waits[0].all = false;                 // the passes wait for the own way in only
            if (mut == 1 && st.op == Op::XINV && st.part == 0) st.waits.clear();          // the inverse x pass does not wait for the way back
            if (mut == 2 && st.op == Op::EXCH_BACK) st.waits.clear();                     // the way back does not wait for the passes
        }
        if (mut == 3) std::swap(s.front(), s.back());                                     // a wait ahead of its record
        if (mut == 4) for (Step& st : s) if (st.op == Op::EXCH_IN) st.waits.clear();      // the way in does not wait for the previous apply to drain
        CHECK(check_pipeline(s, 2, 2, "broken", true) > 0, "broken schedule %d passes the check", mut);
    }
    printf("messages checked: %ld, pipeline schedules checked: %ld, failures: %d\n", checked, configs, bad);
    return bad ? 1 : 0;
}
#endif
