// frame_book.h — the one record of a context's frames in flight, and so of what the next
// update must wait for. Pure host code without a HIP dependency, tested on its own
// (tests/cpp/frame_book_test.cpp). The context reports what happened, one method per event,
// and asks the book what the next frame needs (begin); it keeps the streams, events and
// sequence words themselves and executes the plan (ddgi_frame.cpp).
// The per-frame buffers the traversal writes come in two sets (slot table, slot order,
// sample directions, hit records, work counters); frame n uses set n & 1. A pipelined frame's
// traversal part (slot table, primary traversal, probe offsets) runs on the traversal stream
// as soon as frame n - 2, the previous user of its set, is done, after frame n - 1's offsets,
// beside frame n - 1's caller part (shadow rays, shading, probe update) on the caller's
// stream. A frame may be pipelined when the previous context operation was an update with
// the same sample count and neither is instrumented; every other frame runs serially on the
// caller's stream.
// Two ways to order the streams: device sequence words (k_seq_signal / k_seq_wait: word
// "trace" = the last frame whose traversal part is done, word "main" = the last frame whose
// caller part is done, both counted by seqN) or events (evTraced, evFrameDone[set]). A frame
// is sequenced by words when it is pipelined and words are on; a set remembers how the frame
// that last used it was marked done. Z-slab exchanges count on a word of their own.
#pragma once

#include <cstdint>

namespace ark {

// What updateImpl executes for one frame
struct FramePlan {
    enum Reuse : uint8_t { None, Word, Event };
    bool pipe = false;          // the traversal part runs on the traversal stream (else in line on the caller's)
    uint32_t b = 0;             // the frame's buffer set
    bool seq = false;           // the streams are ordered by sequence words (else events); only when pipe
    uint32_t seqN = 0;          // the frame's sequence number when seq, else 0
    Reuse reuse = None;         // what the traversal part waits for before it reuses set b:
    uint32_t reuseSeq = 0;      //   Word: main >= reuseSeq; Event: evFrameDone[b]
    bool waitOtherDone = false; // and evFrameDone[b ^ 1]: a serial previous frame wrote its offsets on the caller's stream
};

class FrameBook {
public:
    bool pipelining = true; // ARK_DDGI_FLAG_SERIAL_FRAMES clears it: every update runs serially

    // The next update's plan, for R rays per probe; instrumented updates (per-kernel events,
    // counters) run serially. Consumes a sequence number when the plan's seq is set and
    // changes nothing else: an update that fails before finished() leaves the book so.
    FramePlan begin(uint32_t R, bool instrumented)
    {
        FramePlan p;
        p.pipe = pipelining && pipeReady && !instrumented && R == prevR;
        p.b = parity;
        p.seq = p.pipe && seqSync;
        p.seqN = p.seq ? ++frameSeq : 0u;
        if (p.pipe && setSeqValid[p.b]) {
            p.reuse = FramePlan::Word;
            p.reuseSeq = setSeq[p.b];
        } else if (p.pipe && frameDoneValid[p.b]) {
            p.reuse = FramePlan::Event;
        }
        p.waitOtherDone = p.pipe && !prevPipelined && frameDoneValid[p.b ^ 1u];
        return p;
    }
    // The plan's frame is enqueued whole: its set is marked done by word (seq) or by its event
    void finished(const FramePlan& p, uint32_t R)
    {
        if (p.seq) setSeq[p.b] = p.seqN;
        setSeqValid[p.b] = p.seq;
        frameDoneValid[p.b] = true;
        lastMain = p.seq ? p.seqN : 0u;
        parity = p.b ^ 1u;
        pipeReady = true;
        prevR = R;
        prevPipelined = p.pipe;
        lastParity = p.b;
    }
    // A context operation other than an update wrote what the traversal part reads (a scene,
    // a resource, a loaded or cleared history, the caller's own writes): the next update's
    // traversal waits for it, in line on the caller's stream
    void externalWrite() { pipeReady = false; }
    // A sequence-word wait gave up (checkSequencing drained the device): events from here
    // on, the next frame serial
    void timedOut()
    {
        seqSync = false;
        pipeReady = false;
        ++seqTimeouts;
    }
    void setSequencing(bool words) { seqSync = words; }
    bool words() const { return seqSync; }
    uint32_t timeouts() const { return seqTimeouts; }
    uint32_t nextSet() const { return parity; }
    uint32_t lastSet() const { return lastParity; }     // the last update's (debug hit records)
    uint32_t lastMainSeq() const { return lastMain; }   // the last update's sequence number on word main (0: not sequenced)

    // Z-slab exchanges (exchange_end, update_exchanged): the ending exchange takes the next
    // number, is pending once its end is enqueued (signalled on the exchange word, or
    // evExchangeDone recorded), and the next exchanged update waits for it before shading;
    // it stays pending until such an update succeeded.
    uint32_t exchangeNumber() { return ++exchSeq; }
    void exchangeEnded(uint32_t n) { pendingExchange = n; }
    uint32_t exchangePending() const { return pendingExchange; }
    void exchangeWaited() { pendingExchange = 0; }

private:
    bool pipeReady = false;     // the previous context operation was an update
    uint32_t parity = 0;        // buffer set of the next update
    uint32_t prevR = 0;
    bool prevPipelined = false; // the previous update's offsets ran on the traversal stream
    bool frameDoneValid[2] = { false, false };
    bool seqSync = true;        // words (ark_ddgi_set_sequencing(ctx, 0, ...): events throughout)
    uint32_t frameSeq = 0;
    uint32_t setSeq[2] = { 0, 0 }; // the frame that last used buffer set b, when it was sequenced by words
    bool setSeqValid[2] = { false, false }; // (else its evFrameDone[b] is recorded)
    uint32_t seqTimeouts = 0;   // timeouts reported so far
    uint32_t lastMain = 0;
    uint32_t exchSeq = 0;         // exchanges ended so far
    uint32_t pendingExchange = 0; // the exchange the next update_exchanged waits for before shading
    uint32_t lastParity = 0;
};

} // namespace ark
