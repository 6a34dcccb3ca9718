// vertex_dirty_test.cpp — csrc/vertex_dirty.h on its own (tests/test_vertex_dirty_sanitizers.py
// builds it with -fsanitize=address,undefined): which instances a vertex range touches over
// a table of mesh layouts, and the version / dirty bookkeeping over a simulated chain of
// refits and one install, against a model that keeps, per geometry copy and for the shared
// boxes scratch, the vertex generation every instance's data was derived from.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vertex_dirty.h"

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

struct Case {
    const char* name;
    uint32_t first, count;
    std::vector<uint8_t> want; // per instance
};

// meshes: 0 [0, 9], 1 [10, 19] (abuts 0), 2 [15, 30] (overlaps 1), 3 [100, 100] (one vertex),
// 4 unused [40, 49]; instances: 0 -> mesh 0, 1 -> mesh 1, 2 -> mesh 2, 3 -> mesh 0 (shared),
// 4 -> mesh 3
static void touchedTable()
{
    std::vector<MeshSpan> spans(5);
    spans[0] = { 0, 9, true };
    spans[1] = { 10, 9, true };
    spans[2] = { 15, 15, true };
    spans[3] = { 100, 0, true };
    spans[4] = { 40, 9, false };
    const std::vector<uint32_t> instMesh = { 0, 1, 2, 0, 3 };
    const uint64_t pool = 101;
    const std::vector<Case> cases = {
        { "disjoint: between the spans", 31, 9, { 0, 0, 0, 0, 0 } },
        { "disjoint: an unused mesh's vertices", 40, 10, { 0, 0, 0, 0, 0 } },
        { "inside mesh 0: both of its instances", 3, 2, { 1, 0, 0, 1, 0 } },
        { "abutting: the last vertex of mesh 0", 9, 1, { 1, 0, 0, 1, 0 } },
        { "abutting: the first vertex of mesh 1", 10, 1, { 0, 1, 0, 0, 0 } },
        { "abutting: across the seam", 9, 2, { 1, 1, 0, 1, 0 } },
        { "overlapping spans: both meshes", 15, 5, { 0, 1, 1, 0, 0 } },
        { "overlapping spans: only the later mesh", 20, 11, { 0, 0, 1, 0, 0 } },
        { "ends one before a span", 90, 10, { 0, 0, 0, 0, 0 } },
        { "a single-vertex mesh", 100, 1, { 0, 0, 0, 0, 1 } },
        { "an empty range inside a span", 5, 0, { 0, 0, 0, 0, 0 } },
        { "an empty range at the pool's end", 101, 0, { 0, 0, 0, 0, 0 } },
        { "the whole pool", 0, 101, { 1, 1, 1, 1, 1 } },
    };
    for (const Case& c : cases) {
        CHECK(vertexRangeInPool(c.first, c.count, pool), "%s: in the pool", c.name);
        std::vector<uint8_t> got;
        touchedInstances(spans, instMesh, c.first, c.count, got);
        CHECK(got == c.want, "%s", c.name);
    }
    // ranges past the pool
    CHECK(!vertexRangeInPool(101, 1, pool), "one past the end");
    CHECK(!vertexRangeInPool(95, 7, pool), "runs over the end");
    CHECK(!vertexRangeInPool(0xffffffffu, 0xffffffffu, pool), "no 32-bit wrap");
    CHECK(!vertexRangeInPool(102, 0, pool), "an empty range past the end");
    CHECK(vertexRangeInPool(0, 0, 0), "an empty range of an empty pool");
    // several ranges accumulate; an instance of a mesh index outside the table is skipped
    std::vector<uint8_t> acc;
    touchedInstances(spans, instMesh, 0, 1, acc);
    touchedInstances(spans, instMesh, 100, 1, acc);
    CHECK((acc == std::vector<uint8_t> { 1, 0, 0, 1, 1 }), "two ranges");
    std::vector<uint8_t> odd;
    touchedInstances(spans, { 0, 9 }, 0, 5, odd);
    CHECK((odd == std::vector<uint8_t> { 1, 0 }), "unknown mesh");
    // covered spans: the range's bounds replace the box
    CHECK(spanCovered(spans[0], 0, 10) && spanCovered(spans[0], 0, 50) && !spanCovered(spans[0], 1, 20) && !spanCovered(spans[0], 0, 9), "covered");
    CHECK(!spanCovered(spans[4], 40, 10) && !spanCovered(spans[0], 0, 0), "unused / empty never covered");
    // a negative first_vertex (the ABI's int32) never wraps
    MeshSpan neg { -5, 9, true };
    CHECK(spanTouched(neg, 0, 1) && spanTouched(neg, 4, 1) && !spanTouched(neg, 5, 1), "negative first");
}

// The model: gen[i] the generation of instance i's vertices in the pool; rec[slot][i] the
// generation copy `slot`'s records of i were derived from; box[i] the generation the shared
// boxes scratch above i was. A refit of `slot` re-derives exactly the instances the
// bookkeeping calls dirty; afterwards the slot's records and the scratch must all be current.
struct Model {
    size_t n;
    std::vector<uint64_t> gen, box;
    std::vector<uint64_t> rec[3];
    VertexVersions v;
    uint64_t next = 0;
    explicit Model(size_t n) : n(n), gen(n, 0), box(n, 0)
    {
        for (auto& r : rec) r.assign(n, 0);
    }
    void update(const std::vector<uint8_t>& touched)
    {
        v.begin(n);
        ++next;
        for (size_t i = 0; i < n; ++i)
            if (touched[i]) {
                v.touch(i);
                gen[i] = next;
            }
    }
    // the refit of `slot`; returns how many instances it re-derived
    size_t refit(int slot, const char* what)
    {
        size_t dirty = 0;
        for (size_t i = 0; i < n; ++i) {
            if (v.dirty(i, slot)) {
                rec[slot][i] = gen[i];
                box[i] = gen[i];
                ++dirty;
            }
            CHECK(rec[slot][i] == gen[i], "%s: slot %d keeps stale records of instance %zu", what, slot, i);
            CHECK(box[i] == gen[i], "%s: the scratch above instance %zu is stale", what, i);
        }
        v.refitted(slot);
        return dirty;
    }
    void copy(int dst, int src)
    {
        rec[dst] = rec[src];
        v.copied(dst, src);
    }
};

static void versionChain()
{
    const size_t n = 70; // ids 3 and 67 alias mod 64: the versions are per instance
    Model m(n);
    std::vector<uint8_t> none(n, 0), a(n, 0), b(n, 0);
    a[3] = a[67] = 1;
    b[5] = 1;
    CHECK(!m.v.inUse(), "unused at first");
    for (size_t i = 0; i < n + 3; ++i) CHECK(!m.v.dirty(i, 0) && !m.v.dirty(i, 2), "nothing dirty before the first update");
    // the copies rotate 1, 2, 0, 1, ... as the store's do (front 0 at first)
    int slot = 1;
    auto next = [&] { const int s = slot; slot = (slot + 1) % 3; return s; };
    m.update(a);
    CHECK(m.v.inUse(), "in use");
    CHECK(m.refit(next(), "deform once") == 2, "the touched pair only");
    // three refits without an update: each remaining copy catches up once, then nothing is dirty
    CHECK(m.refit(next(), "catch-up 1") == 2, "slot 2 saw the old vertices");
    CHECK(m.refit(next(), "catch-up 2") == 2, "slot 0 saw the old vertices");
    CHECK(m.refit(next(), "catch-up 3") == 0, "every copy current");
    // updates in a row: every refit's target is two updates behind
    for (int k = 0; k < 7; ++k) {
        m.update(k % 2 ? b : a);
        m.refit(next(), "updates in a row");
    }
    // an update no refit follows at once (a failed call), then one of another instance
    m.update(a);
    m.update(b);
    CHECK(m.refit(next(), "after a skipped refit") == 3, "both updates' instances");
    m.refit(next(), "then");
    m.refit(next(), "then");
    CHECK(m.refit(next(), "settled") == 0, "settled");
    // an install: a job snapshots the front copy, two updates come in, the front copy gets
    // the snapshot's records back and is refitted forward (every instance re-derived); the
    // spares are dropped and copied from the front one by the next refit
    const int front = (slot + 2) % 3;
    const std::vector<uint64_t> snapshot = m.rec[front];
    m.update(a);
    m.refit(next(), "while the job runs");
    m.update(b);
    m.refit(next(), "while the job runs");
    const int front2 = (slot + 2) % 3;
    m.rec[front2] = snapshot;
    for (size_t i = 0; i < n; ++i) m.rec[front2][i] = m.box[i] = m.gen[i]; // the forward refit: all dirty
    m.v.installed(front2, true);
    for (size_t i = 0; i < n; ++i) CHECK(!m.v.dirty(i, front2), "the installed copy is current (%zu)", i);
    const int tgt = next();
    m.copy(tgt, front2);
    CHECK(m.refit(tgt, "first refit after the install") == 0, "copied from the current front");
    m.update(a);
    m.copy(slot, tgt);
    CHECK(m.refit(next(), "an update after the install") == 2, "the pair");
    // an install without a forward refit changes nothing
    VertexVersions before = m.v;
    m.v.installed(0, false);
    CHECK(before.copy[0] == m.v.copy[0] && before.scratch == m.v.scratch, "no forward refit");
    // a scene with another instance count starts over
    m.v.begin(4);
    CHECK(m.v.inst.size() == 4 && !m.v.dirty(9, 0), "resized");
}

int main()
{
    touchedTable();
    versionChain();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
