// copy_book_test.cpp — csrc/copy_book.h on its own (tests/test_copy_book_sanitizers.py builds
// it with -fsanitize=address,undefined): the record of what the three geometry copies hold,
// driven through the store's lifecycle against a model of the device state. The model
// extends vertex_dirty_test.cpp's: per instance a pose and a vertex generation; per slot
// the (pose, generation) its records of every instance were derived from and the inflation
// its boxes hold; for the shared boxes scratch the same per instance. A refit re-derives
// exactly the instances the book calls dirty (and, as refitBvh does, every box from the
// target's records when the book says `full` or an inflation differs), then checks that the
// target's records and the scratch above every instance are current. It also counts: the
// book must call dirty exactly the instances whose records or scratch are stale.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "copy_book.h"

using namespace ark;

static int failures = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
            ++failures;                                      \
        }                                                    \
    } while (0)

struct Inst {
    float object_to_world[12];
};
using State = std::pair<int, uint64_t>; // the pose and the vertex generation something was derived from
static const State kGarbage { -1, ~0ull };

struct Model {
    size_t n = 0;
    std::vector<int> pose;     // what the caller asks for next
    std::vector<uint64_t> gen; // the vertices in the pool
    std::vector<State> rec[3], box;
    std::vector<float> boxInfl; // the inflation of the scratch above each instance
    float recInfl[3] = { 0, 0, 0 };
    uint64_t nextGen = 0;
    CopyBook book;

    static Inst inst(int pose)
    {
        Inst q {};
        q.object_to_world[0] = q.object_to_world[5] = q.object_to_world[10] = 1.0f;
        q.object_to_world[3] = static_cast<float>(pose);
        return q;
    }
    std::vector<Inst> insts() const
    {
        std::vector<Inst> v(n);
        for (size_t i = 0; i < n; ++i) v[i] = inst(pose[i]);
        return v;
    }
    void setScene(size_t count)
    {
        n = count;
        pose.assign(n, 0);
        gen.assign(n, 0);
        nextGen = 0;
        for (auto& r : rec) r.assign(n, kGarbage);
        rec[0].assign(n, State { 0, 0 });
        box.assign(n, kGarbage); // no scratch before the first refit
        boxInfl.assign(n, -1.0f);
        recInfl[0] = recInfl[1] = recInfl[2] = 0.0f;
        const std::vector<Inst> v = insts();
        book.newScene(v.data(), n);
        CHECK(book.front() == 0 && book.target() == 1 && book.order[2] == 2 && book.full && !book.targetValid() && !book.vtx.inUse(), "a new scene's book");
    }
    // a vertex update: the pool holds the touched instances' new vertices whatever follows
    void deform(const std::vector<size_t>& touched)
    {
        std::vector<uint8_t> flags(n, 0);
        ++nextGen;
        for (size_t i : touched) {
            flags[i] = 1;
            gen[i] = nextGen;
        }
        book.vertexUpdate(flags);
    }
    void copyIfInvalid()
    {
        const int t = book.target(), f = book.front();
        if (book.targetValid()) return;
        rec[t] = rec[f];
        recInfl[t] = recInfl[f];
        book.copied();
        CHECK(book.targetValid(), "valid once copied");
    }
    // what refitBvh and k_refit_nodes do with the book's answers, on `slot`
    size_t derive(CopyBook::Refit which, int slot, float infl, const std::vector<Inst>& v, const char* what)
    {
        size_t dirty = 0, needed = 0;
        CHECK(book.inflation(slot, 0) == recInfl[slot], "%s: the book's held inflation of slot %d", what, slot);
        const bool every = book.full || infl != book.inflation(slot, 0) || boxInfl.empty() || infl != boxInfl[0];
        for (size_t i = 0; i < n; ++i) {
            const State cur { pose[i], gen[i] };
            needed += rec[slot][i] != cur || box[i] != cur;
            if (book.dirty(which, i, v[i].object_to_world)) {
                rec[slot][i] = box[i] = cur;
                boxInfl[i] = infl;
                ++dirty;
            }
            if (every) {
                box[i] = rec[slot][i];
                boxInfl[i] = infl;
            }
        }
        book.inflation(slot, 0) = recInfl[slot] = infl;
        for (size_t i = 0; i < n; ++i) {
            const State cur { pose[i], gen[i] };
            CHECK(rec[slot][i] == cur, "%s: slot %d keeps stale records of instance %zu", what, slot, i);
            CHECK(box[i] == cur, "%s: the scratch above instance %zu is stale", what, i);
            CHECK(boxInfl[i] == infl, "%s: the scratch above instance %zu is of another inflation", what, i);
        }
        // exactly the stale ones - unless the scratch is unknown (`full` after a failure or an
        // install), which the nodes' full pass repairs, not the instances' flags
        if (which == CopyBook::Target && !every) CHECK(dirty == needed, "%s: %zu dirty, %zu stale", what, dirty, needed);
        return dirty;
    }
    // the refit of the next target to the poses asked for; returns how many instances it re-derived
    size_t refit(const char* what, float infl = 1.0f)
    {
        const std::vector<Inst> v = insts();
        copyIfInvalid();
        const int t = book.target(), f = book.front(), l = book.order[2];
        const size_t dirty = derive(CopyBook::Target, t, infl, v, what);
        book.refitted(v.data(), n);
        CHECK(book.front() == t && book.target() == l && book.order[2] == f && !book.full, "%s: the rotation", what);
        return dirty;
    }
    // a refit that fails after the copy, the target half written
    void failedRefit()
    {
        copyIfInvalid();
        const int t = book.target();
        for (size_t i = 0; i < n; i += 2) rec[t][i] = box[i] = kGarbage;
        book.targetUnknown();
        CHECK(!book.targetValid() && book.full && book.target() == t, "the target is unknown, no rotation");
    }
    // An install: the front copy gets `snapshot`'s records back in a new topology (the
    // scratch is of the old one, the spares are dropped), refitted forward when refits came
    // in since the snapshot
    void install(const std::vector<State>& snapshot, bool forward, float infl = 1.0f)
    {
        const int f = book.front();
        rec[f] = snapshot;
        box.assign(n, kGarbage);
        rec[book.order[1]].assign(n, kGarbage);
        rec[book.order[2]].assign(n, kGarbage);
        book.installed(forward);
        CHECK(book.full && !book.targetValid() && !book.slot[book.order[2]].valid && book.front() == f, "an install drops the spares");
        if (forward) CHECK(derive(CopyBook::Forward, f, infl, insts(), "forward refit") == n, "the forward refit re-derives every instance");
        CHECK(book.full, "the first refit after an install reaches every node");
    }
};

// the sequences of tests/test_gpu_refit_sequences.py, on 70 instances (ids 3 and 67 alias mod 64)
static void sequences()
{
    Model m;
    m.setScene(70);
    const size_t a = 3, b = 67, far = 40;
    auto warmUp = [&] {
        for (int k = 0; k < 3; ++k) {
            m.pose[far] += 1;
            m.refit("warm-up");
        }
        for (int k = 0; k < 3; ++k) CHECK(m.refit("settling") == (k < 2 ? 1u : 0u), "the other two copies catch up with `far`, then nothing");
    };
    warmUp();
    CHECK(m.refit("settled") == 0, "a settled book reports zero dirty");
    // 1: a few of more than 64 moving
    m.pose[a] = 10;
    CHECK(m.refit("a moves") == 1, "one");
    m.pose[b] = 20;
    CHECK(m.refit("b moves") == 2, "b, and a in a copy that never saw it move");
    CHECK(m.refit("rest") == 2, "both in the third copy");
    CHECK(m.refit("rest") == 1, "b in the first");
    CHECK(m.refit("rest") == 0 && m.refit("rest") == 0, "settled");
    // 2: nudge and return. The nudge's target holds the nudged pose, the return's the scratch
    // of it: one dirty each, and one more when the nudge's target comes round again
    m.pose[a] = 11;
    CHECK(m.refit("nudge") == 1, "the nudge");
    m.pose[a] = 10;
    CHECK(m.refit("return") == 1, "the target holds the pose, the scratch does not");
    CHECK(m.refit("after the return") == 0, "this copy and the scratch hold it");
    CHECK(m.refit("after the return") == 1, "the nudge's copy");
    CHECK(m.refit("after the return") == 0, "settled");
    // 3: a loop of period 3: every target already holds the pose asked for, the scratch never
    for (int k = 0; k < 9; ++k) {
        m.pose[a] = 30 + k % 3;
        CHECK(m.refit("loop of period 3") == 1, "step %d", k);
    }
    // 4: an inflation change reaches every node in each copy once
    for (int k = 0; k < 3; ++k) m.refit("settle the loop");
    CHECK(m.refit("inflation doubles", 2.0f) == 0, "no instance is dirty, every box is re-derived");
    m.pose[b] = 21;
    CHECK(m.refit("second copy at the new inflation", 2.0f) == 1, "b");
    m.refit("third", 2.0f);
    m.refit("partial again", 2.0f);
    m.refit("and back", 1.0f);
    // mixed pose and vertex updates
    for (int k = 0; k < 8; ++k) {
        if (k % 2) m.deform({ a, b });
        if (k % 3 == 0) m.pose[far] += 1;
        if (k == 5) m.deform({ far });
        m.refit("mixed");
    }
    for (int k = 0; k < 3; ++k) m.refit("settle");
    CHECK(m.refit("settled") == 0, "settled after the mix");
}

static void failures_()
{
    Model m;
    m.setScene(9);
    for (int k = 0; k < 4; ++k) {
        m.pose[1] += 1;
        m.refit("warm-up");
    }
    // a refit that fails after the copy: the next one copies anew and reaches every node
    m.pose[2] = 5;
    m.failedRefit();
    CHECK(m.refit("after a failed refit") >= 1, "instance 2 at least");
    for (int k = 0; k < 3; ++k) m.refit("settle");
    CHECK(m.refit("settled") == 0, "settled after the failure");
    // a failed vertex staging: the pool holds the new vertices, no copy does
    m.deform({ 0, 4 });
    m.book.targetUnknown();
    for (int k = 0; k < 3; ++k) CHECK(m.refit("after a failed staging") >= 2, "the touched pair is dirty for all three copies (%d)", k);
    CHECK(m.refit("settled") == 0, "settled after the failed staging");
}

static void installs()
{
    Model m;
    m.setScene(12);
    for (int k = 0; k < 4; ++k) {
        m.pose[k % 3] += 1;
        m.refit("warm-up");
    }
    // with a forward refit: a pose and a vertex update came in since the snapshot
    std::vector<State> snapshot = m.rec[m.book.front()];
    m.pose[7] = 3;
    m.refit("while the job runs");
    m.deform({ 8 });
    m.refit("while the job runs");
    m.install(snapshot, true);
    CHECK(m.refit("first dropped spare") == 0, "copied from the current front");
    CHECK(!m.book.targetValid(), "the second spare is still dropped");
    m.pose[9] = 4;
    CHECK(m.refit("second dropped spare") == 1, "copied too: only what moved");
    CHECK(m.refit("third") == 1 && m.refit("fourth") == 1 && m.refit("settled") == 0, "the other copies catch up");
    // without: nothing came in since the snapshot
    snapshot = m.rec[m.book.front()];
    m.install(snapshot, false);
    m.deform({ 2 });
    CHECK(m.refit("first dropped spare") >= 1, "the update, every node");
    CHECK(m.refit("second dropped spare") == 0, "copied from the current front");
    CHECK(m.refit("the installed copy") == 1 && m.refit("settled") == 0, "it saw the old vertices");
    // a new scene with another instance count starts over
    m.setScene(5);
    m.pose[4] = 1;
    CHECK(m.refit("first refit of a new scene") == 1, "one moved; every node (full)");
    m.deform({ 0 });
    CHECK(m.refit("second") == 1 && m.book.vtx.inst.size() == 5, "the second spare is copied from the front one too: the update only; resized");
}

int main()
{
    sequences();
    failures_();
    installs();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
