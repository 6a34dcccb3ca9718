// frame_book_test.cpp — the record of the frames in flight (frame_book.h: FrameBook) against
// the rule it replaced, against a model of the two queues, and as a table of named cases.
// Stand-alone: built and run under AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_frame_book.py. No GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "frame_book.h"

using namespace ark;

namespace {

// the events of the sweep
enum Event { U64, U128, UInstrumented, ExternalWrite, WordsOn, WordsOff, Timeout, Exchanged, kEvents };
const char* const kEventName[kEvents] = { "update(64)", "update(128)", "instrumented update", "external write", "words on", "words off", "timeout", "exchange end + exchanged update" };
constexpr int kMaxEvents = 7;

int g_seq[kMaxEvents], g_len = 0; // the sequence being run (reported by CHECK)

void printSequence()
{
    std::printf("  after:");
    for (int i = 0; i < g_len; ++i) std::printf(" %s;", kEventName[g_seq[i]]);
    std::printf("\n");
}

#define CHECK(x)                                                            \
    do {                                                                    \
        if (!(x)) {                                                         \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);     \
            printSequence();                                                \
            return 1;                                                       \
        }                                                                   \
    } while (0)

// --- 1. the rule before the book --------------------------------------------------------
// The fields of ArkDdgiCtx and the lines of ark_ddgi.cpp that decided a frame's streams and
// waits at commit cd3c5a5 ("Skin and morph deforming meshes on the device"), copied
// literally with `ctx->` dropped; a launch or an event call is replaced by the plan field it
// stands for.
struct Parent {
    bool pipelining = true;
    bool timing = false, counting = false;
    bool pipeReady = false;
    uint32_t parity = 0;
    uint32_t prevR = 0;
    bool prevPipelined = false;
    bool frameDoneValid[2] = { false, false };
    bool seqSync = true;
    uint32_t frameSeq = 0;
    uint32_t setSeq[2] = { 0, 0 };
    bool setSeqValid[2] = { false, false };
    uint32_t seqTimeouts = 0;
    uint32_t lastMainSeq = 0;
    uint32_t exchSeq = 0;
    uint32_t pendingExchange = 0;
    uint32_t lastParity = 0;

    // updateImpl, down to the waits ahead of k_probe_slots
    FramePlan updateHead(uint32_t R)
    {
        FramePlan q;
        const bool timing = this->timing;
        const bool count = this->counting;
        const bool pipe = pipelining && pipeReady && !timing && !count && R == prevR;
        const uint32_t b = parity;
        const bool seq = pipe && seqSync;
        const uint32_t seqN = seq ? ++frameSeq : 0u;
        if (pipe && setSeqValid[b]) { q.reuse = FramePlan::Word; q.reuseSeq = setSeq[b]; } // launch_seq_wait(seqMain, setSeq[b], ..., ts)
        else if (pipe && frameDoneValid[b]) q.reuse = FramePlan::Event;                     // hipStreamWaitEvent(ts, evFrameDone[b], 0)
        if (pipe && !prevPipelined && frameDoneValid[b ^ 1u]) q.waitOtherDone = true;        // hipStreamWaitEvent(ts, evFrameDone[b ^ 1u], 0)
        q.pipe = pipe;
        q.b = b;
        q.seq = seq;
        q.seqN = seqN;
        return q;
    }
    // updateImpl, from the done signal to its return
    void updateTail(bool pipe, uint32_t b, bool seq, uint32_t seqN, uint32_t R)
    {
        if (seq) {
            setSeq[b] = seqN;
            setSeqValid[b] = true;
        } else {
            setSeqValid[b] = false;
        }
        frameDoneValid[b] = true;
        lastMainSeq = seq ? seqN : 0u;
        parity = b ^ 1u;
        pipeReady = true;
        prevR = R;
        prevPipelined = pipe;
        lastParity = b;
    }
    // set_scene, share_scene, write, load_state, reset_history, mark_external_write
    void externalWrite() { pipeReady = false; }
    // checkSequencing, once the flag is seen and the device drained
    void timedOut()
    {
        seqSync = false;
        pipeReady = false;
        ++seqTimeouts;
    }
    void setSequencing(int device_sequence_words) { seqSync = device_sequence_words != 0; }
    // exchange_end: the number signalled (or evExchangeDone recorded), then pending
    uint32_t exchangeEnd()
    {
        const uint32_t n = ++exchSeq;
        pendingExchange = n;
        return n;
    }
    // update_exchanged: around updateImpl
    uint32_t exchangedWait() const { const uint32_t wait = pendingExchange; return wait; }
    void exchangedOk() { pendingExchange = 0; }
};

bool samePlan(const FramePlan& a, const FramePlan& b)
{
    return a.pipe == b.pipe && a.b == b.b && a.seq == b.seq && a.seqN == b.seqN && a.reuse == b.reuse && a.reuseSeq == b.reuseSeq && a.waitOtherDone == b.waitOtherDone;
}

bool sameState(const Parent& p, const FrameBook& k)
{
    return p.parity == k.nextSet() && p.lastParity == k.lastSet() && p.lastMainSeq == k.lastMainSeq() && p.seqTimeouts == k.timeouts() &&
           p.pendingExchange == k.exchangePending() && p.seqSync == k.words();
}

// --- 2. the two queues --------------------------------------------------------------------
// What the context enqueues for a plan, on the caller's stream, the traversal stream and the
// exchange stream, and what happens before what: stream order, event record -> wait, word
// signal -> wait (a wait for v is met by any signal of at least v). An operation is the n-th
// of its stream; a clock says how many operations of each stream happen before a point.
enum Stream { Caller, Trav, Exch, kStreams };
enum WordId { WTrace, WMain, WExchange, kWords };

struct Clock {
    int c[kStreams] = { 0, 0, 0 };
    void join(const Clock& o) { for (int i = 0; i < kStreams; ++i) c[i] = std::max(c[i], o.c[i]); }
};

struct Op {
    int stream = 0, index = 0; // index 0: none
    Clock at;                  // what happens before it, itself included
};

struct Model {
    Clock now[kStreams];   // what the next operation of a stream follows
    int count[kStreams] = { 0, 0, 0 };
    struct Ev { bool recorded = false; Clock at; } evTraced, evFrameDone[2], evExchangeDone;
    struct Signal { uint32_t v = 0; Clock at; };
    struct Word { Signal s[kMaxEvents + 1]; int n = 0; } word[kWords];
    Op lastCaller[2];      // the caller part of the last frame that used a set
    Op prevOffsets;        // the previous frame's offsets write
    uint32_t drainedMain = 0; // word main's last value signalled before the last drain

    Op enqueue(int s)
    {
        Op o;
        o.stream = s;
        o.index = ++count[s];
        now[s].c[s] = o.index;
        o.at = now[s];
        return o;
    }
    static bool follows(const Op& later, const Op& earlier) { return later.at.c[earlier.stream] >= earlier.index; }
    void record(Ev& e, int s) { e.recorded = true; e.at = now[s]; }
    int waitEvent(int s, const Ev& e)
    {
        CHECK(e.recorded); // (a wait for an event never recorded orders nothing)
        now[s].join(e.at);
        return 0;
    }
    int signal(int w, uint32_t v, int s)
    {
        Word& W = word[w];
        CHECK(W.n == 0 || v > W.s[W.n - 1].v); // a word's signalled values strictly increase
        CHECK(W.n < kMaxEvents + 1);
        W.s[W.n].v = v;
        W.s[W.n].at = enqueue(s).at;
        ++W.n;
        return 0;
    }
    int waitWord(int s, int w, uint32_t v)
    {
        // met by whichever signal of at least v runs first: only what every one of them follows
        const Word& W = word[w];
        bool any = false;
        Clock least;
        for (int i = 0; i < W.n; ++i) {
            if (W.s[i].v < v) continue;
            if (!any) least = W.s[i].at;
            else for (int k = 0; k < kStreams; ++k) least.c[k] = std::min(least.c[k], W.s[i].at.c[k]);
            any = true;
        }
        CHECK(any); // the value's signal was enqueued earlier in host order
        now[s].join(least);
        return 0;
    }
    // checkSequencing's hipDeviceSynchronize
    void drain()
    {
        Clock all;
        for (int i = 0; i < kStreams; ++i) all.c[i] = count[i];
        for (Clock& n : now) n = all;
        drainedMain = word[WMain].n ? word[WMain].s[word[WMain].n - 1].v : 0u;
    }
    // updateImpl's enqueue order for plan p; exchange n (0: none) awaited before shading
    int frame(const FramePlan& p, bool exchangeByWord, uint32_t exchange)
    {
        const int ts = p.pipe ? Trav : Caller;
        if (p.reuse == FramePlan::Word) { if (waitWord(ts, WMain, p.reuseSeq)) return 1; }
        else if (p.reuse == FramePlan::Event) { if (waitEvent(ts, evFrameDone[p.b])) return 1; }
        if (p.waitOtherDone && waitEvent(ts, evFrameDone[p.b ^ 1u])) return 1;
        const Op trav = enqueue(ts); // slot table, primary traversal
        // follows the caller part of the last frame that used its buffer set
        CHECK(lastCaller[p.b].index == 0 || follows(trav, lastCaller[p.b]));
        // follows the previous frame's offsets write, wherever that ran
        CHECK(prevOffsets.index == 0 || follows(trav, prevOffsets));
        Op offsets;
        if (p.pipe) {
            offsets = enqueue(Trav);
            if (p.seq) { // tracedSync
                if (signal(WTrace, p.seqN, Trav) || waitWord(Caller, WTrace, p.seqN)) return 1;
            } else {
                record(evTraced, Trav);
                if (waitEvent(Caller, evTraced)) return 1;
            }
        }
        if (exchange && (exchangeByWord ? waitWord(Caller, WExchange, exchange) : waitEvent(Caller, evExchangeDone))) return 1;
        const Op caller = enqueue(Caller); // shadow rays, shading, (serial: offsets,) probe update
        CHECK(follows(caller, trav));      // follows its own traversal part
        if (!p.pipe) offsets = caller;
        if (p.seq) { if (signal(WMain, p.seqN, Caller)) return 1; }
        else record(evFrameDone[p.b], Caller);
        lastCaller[p.b] = caller;
        prevOffsets = offsets;
        return 0;
    }
    int exchangeEnd(bool byWord, uint32_t n)
    {
        enqueue(Exch); // the exchange itself
        if (byWord) return signal(WExchange, n, Exch);
        record(evExchangeDone, Exch);
        return 0;
    }
};

// one state of the sweep: the restatement, the book, the queues, and what the next frame owes
struct World {
    Parent parent;
    FrameBook book;
    Model model;
    uint32_t lastR = 0;
    bool serialDue = true;     // the next frame follows nothing, an external write or a timeout
    bool afterTimeout = false; // a timeout, and words not switched on since
};

long g_steps = 0, g_pipelined = 0, g_wordFrames = 0, g_staleWordWaits = 0;

int update(World& w, uint32_t R, bool instrumented, bool exchanged)
{
    w.parent.counting = instrumented;
    // (update_exchanged chooses word or event before updateImpl runs)
    const bool byWord = w.book.words();
    CHECK(byWord == w.parent.seqSync);
    const uint32_t wait = exchanged ? w.book.exchangePending() : 0u;
    CHECK(!exchanged || wait == w.parent.exchangedWait());
    const FramePlan q = w.parent.updateHead(R);
    const FramePlan p = w.book.begin(R, instrumented);
    CHECK(samePlan(p, q));
    CHECK(sameState(w.parent, w.book)); // begin changed nothing that shows
    // the frame after an external write, an R change, an instrumented request or a timeout is not pipelined
    if (w.serialDue || R != w.lastR || instrumented) CHECK(!p.pipe);
    CHECK(!p.seq || p.pipe);
    CHECK((p.seqN != 0) == p.seq);
    // After a timeout no plan uses words. This holds for the frame's own sequencing (seq) but
    // not for the wait before a buffer set is reused: update(64) x 3, timeout, update(64) x 2
    // - the sixth frame reuses the set of the third, which was marked done by word (main = 2)
    // before the timeout, and so waits for that word. The parent did the same, and the book
    // keeps it: the value was signalled before the timeout's drain (signals are never
    // skipped), so the wait is met at once. That half of the invariant is left out.
    if (w.afterTimeout) {
        CHECK(!p.seq);
        if (p.reuse == FramePlan::Word) {
            CHECK(p.reuseSeq <= w.model.drainedMain);
            ++g_staleWordWaits;
        }
    }
    if (w.model.frame(p, byWord, wait)) return 1;
    w.parent.updateTail(q.pipe, q.b, q.seq, q.seqN, R);
    w.book.finished(p, R);
    if (exchanged) {
        w.parent.exchangedOk();
        w.book.exchangeWaited();
    }
    w.parent.counting = false;
    w.lastR = R;
    w.serialDue = false;
    g_pipelined += p.pipe;
    g_wordFrames += p.seq;
    return 0;
}

int apply(World& w, int e)
{
    switch (e) {
    case U64: if (update(w, 64, false, false)) return 1; break;
    case U128: if (update(w, 128, false, false)) return 1; break;
    case UInstrumented: if (update(w, 64, true, false)) return 1; break;
    case ExternalWrite:
        w.parent.externalWrite();
        w.book.externalWrite();
        w.serialDue = true;
        break;
    case WordsOn:
        w.parent.setSequencing(1);
        w.book.setSequencing(true);
        w.afterTimeout = false;
        break;
    case WordsOff:
        w.parent.setSequencing(0);
        w.book.setSequencing(false);
        break;
    case Timeout:
        w.model.drain();
        w.parent.timedOut();
        w.book.timedOut();
        w.serialDue = true;
        w.afterTimeout = true;
        break;
    case Exchanged: {
        const uint32_t n = w.book.exchangeNumber();
        CHECK(n == w.parent.exchangeEnd());
        CHECK(!w.afterTimeout || !w.book.words());
        if (w.model.exchangeEnd(w.book.words(), n)) return 1;
        w.book.exchangeEnded(n);
        CHECK(sameState(w.parent, w.book));
        if (update(w, 64, false, true)) return 1;
        break;
    }
    }
    CHECK(sameState(w.parent, w.book));
    ++g_steps;
    return 0;
}

int sweepFrom(const World& w, int depth)
{
    if (depth == kMaxEvents) return 0;
    for (int e = 0; e < kEvents; ++e) {
        World next = w;
        g_seq[depth] = e;
        g_len = depth + 1;
        if (apply(next, e)) return 1;
        if (sweepFrom(next, depth + 1)) return 1;
    }
    return 0;
}

int sweep(bool pipelining)
{
    World w;
    w.parent.pipelining = w.book.pipelining = pipelining;
    g_steps = g_pipelined = g_wordFrames = g_staleWordWaits = 0;
    if (sweepFrom(w, 0)) return 1;
    g_len = 0;
    long want = 0, pow = 1;
    for (int d = 1; d <= kMaxEvents; ++d) want += (pow *= kEvents);
    CHECK(g_steps == want); // every sequence of up to 7 of the 8 events
    if (pipelining) {
        CHECK(g_pipelined > 0 && g_wordFrames > 0 && g_wordFrames < g_pipelined);
        CHECK(g_staleWordWaits > 0); // (the sequence named in update() is reached)
    } else {
        CHECK(g_pipelined == 0 && g_wordFrames == 0);
    }
    return 0;
}

// --- 3. named cases ---------------------------------------------------------------------
FramePlan frame(FrameBook& k, uint32_t R, bool instrumented = false)
{
    const FramePlan p = k.begin(R, instrumented);
    k.finished(p, R);
    return p;
}

int table()
{
    using P = FramePlan;
    {
        // the first frame is serial, on set 0, and waits for nothing
        FrameBook k;
        const P p = frame(k, 64);
        CHECK(!p.pipe && !p.seq && p.seqN == 0 && p.b == 0 && p.reuse == P::None && !p.waitOtherDone);
        CHECK(k.nextSet() == 1 && k.lastSet() == 0 && k.lastMainSeq() == 0);
        // the second is pipelined: its set is new, the serial first frame wrote its offsets on the caller's stream
        const P q = frame(k, 64);
        CHECK(q.pipe && q.seq && q.seqN == 1 && q.b == 1 && q.reuse == P::None && q.waitOtherDone);
        // the third reuses set 0, which the serial frame marked done by its event
        const P r = frame(k, 64);
        CHECK(r.pipe && r.seqN == 2 && r.b == 0 && r.reuse == P::Event && !r.waitOtherDone);
        // steady state: the sets alternate, each frame waits for the word of two frames before
        for (uint32_t n = 3; n < 10; ++n) {
            const P s = frame(k, 64);
            CHECK(s.pipe && s.seq && s.seqN == n && s.b == (n & 1u) && s.reuse == P::Word && s.reuseSeq == n - 2 && !s.waitOtherDone);
            CHECK(k.lastMainSeq() == n && k.lastSet() == (n & 1u));
        }
        // an R change: serial, no sequence number consumed; the frame after it is pipelined
        // again, waits for its set's word and for the serial frame's event
        const P c = frame(k, 128);
        CHECK(!c.pipe && !c.seq && c.seqN == 0 && c.b == 0 && c.reuse == P::None && k.lastMainSeq() == 0);
        const P d = frame(k, 128);
        CHECK(d.pipe && d.seqN == 10 && d.b == 1 && d.reuse == P::Word && d.reuseSeq == 9 && d.waitOtherDone);
        const P e = frame(k, 128);
        CHECK(e.pipe && e.seqN == 11 && e.b == 0 && e.reuse == P::Event && !e.waitOtherDone);
        // an instrumented update is serial; so is the frame after an external write
        CHECK(!frame(k, 128, true).pipe);
        CHECK(frame(k, 128).pipe);
        k.externalWrite();
        CHECK(!frame(k, 128).pipe);
    }
    {
        // words off, then on: events while off (a set done by word is still awaited by word), words again after
        FrameBook k;
        for (int i = 0; i < 4; ++i) frame(k, 64); // seq 1..3 on sets 1, 0, 1
        k.setSequencing(false);
        const P a = frame(k, 64); // set 0, done by word 2
        CHECK(a.pipe && !a.seq && a.seqN == 0 && a.reuse == P::Word && a.reuseSeq == 2 && k.lastMainSeq() == 0);
        const P b = frame(k, 64); // set 1, done by word 3
        CHECK(b.pipe && !b.seq && b.reuse == P::Word && b.reuseSeq == 3);
        const P c = frame(k, 64); // set 0, done by event
        CHECK(c.pipe && !c.seq && c.reuse == P::Event);
        k.setSequencing(true);
        const P d = frame(k, 64);
        CHECK(d.pipe && d.seq && d.seqN == 4 && d.reuse == P::Event && k.lastMainSeq() == 4);
        frame(k, 64);
        const P e = frame(k, 64);
        CHECK(e.seq && e.seqN == 6 && e.reuse == P::Word && e.reuseSeq == 4);
    }
    {
        // a timeout: counted, words off, the next frame serial, the one after pipelined with events
        FrameBook k;
        for (int i = 0; i < 3; ++i) frame(k, 64);
        k.timedOut();
        CHECK(k.timeouts() == 1 && !k.words());
        const P a = frame(k, 64);
        CHECK(!a.pipe && !a.seq);
        const P b = frame(k, 64);
        CHECK(b.pipe && !b.seq && b.seqN == 0 && b.waitOtherDone);
        k.timedOut();
        CHECK(k.timeouts() == 2);
    }
    {
        // a serial context never pipelines
        FrameBook k;
        k.pipelining = false;
        for (int i = 0; i < 4; ++i) CHECK(!frame(k, 64).pipe);
    }
    {
        // an exchange stays pending across a failed update (begin without finished) and is
        // cleared by the one that succeeded; a failed begin keeps its sequence number
        FrameBook k;
        frame(k, 64);
        frame(k, 64);
        const uint32_t n = k.exchangeNumber();
        k.exchangeEnded(n);
        CHECK(n == 1 && k.exchangePending() == 1);
        const P lost = k.begin(64, false); // the update failed after this
        CHECK(lost.pipe && lost.seqN == 2 && lost.b == 0);
        CHECK(k.exchangePending() == 1 && k.nextSet() == 0 && k.lastMainSeq() == 1);
        const P again = k.begin(64, false);
        CHECK(again.pipe && again.seqN == 3 && again.b == 0 && again.reuse == lost.reuse);
        k.finished(again, 64);
        k.exchangeWaited();
        CHECK(k.exchangePending() == 0 && k.lastMainSeq() == 3);
        CHECK(k.exchangeNumber() == 2);
    }
    return 0;
}

} // namespace

int main()
{
    if (table()) return 1;
    std::printf("table: OK\n");
    if (sweep(false)) return 1;
    std::printf("serial sweep: OK\n");
    if (sweep(true)) return 1;
    std::printf("sweep: %ld steps, %ld pipelined frames, %ld of them by words: OK\n", g_steps, g_pipelined, g_wordFrames);
    return 0;
}
