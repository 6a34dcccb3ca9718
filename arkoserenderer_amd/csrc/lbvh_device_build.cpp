// lbvh_device_build.cpp — buildLbvhGpu (lbvh_device_build.h) and its traced run against the
// host restatement (include/ark_ddgi_debug.h: ark_ddgi_debug_lbvh_device_parity).
#include "lbvh_device_build.h"

#include <algorithm>
#include <array>
#include <cstring>

#include "../../include/ark_ddgi_debug.h"
#include "bvh8_check.h"
#include "bvh_builder.h"
#include "lbvh_host.h"
#include "sun_bvh.h"

namespace ark {

// The deepest BVH8 the device build installs. The traversal's spill area is sized from the
// installed depth (ensureSpill: depth + 2 - kStackLds entries per lane, DeviceBvh::depth),
// and the deepest tree the host builds hand it is bounded by the BVH2 builder's depth cap
// (BvhBuildOptions::max_depth, 60); a radix tree over coincident centroids can be
// deeper, and such a scene is left to the host build.
constexpr uint32_t kGpuBuildMaxDepth = 60;

bool isDeviceFault(hipError_t e)
{
    return e == hipErrorIllegalAddress || e == hipErrorLaunchFailure || e == hipErrorLaunchTimeOut || e == hipErrorECCNotCorrectable || e == hipErrorAssert ||
           e == hipErrorNoDevice || e == hipErrorInvalidDevice;
}

// What a traced device build keeps on the host (ark_ddgi_debug_lbvh_device_parity): every
// stage's result, downloaded before buildLbvhGpu returns (the stages after a fallback: empty)
struct LbvhGpuTrace {
    LbvhHeader hdr {};                            // as the build uses it (the light build's classCount[0] = prims)
    std::vector<uint32_t> idx, idxSorted, split;  // hdr.prims each (split: set at the internal indices of each class range)
    // the SAH pass (LbvhGpuBuild::sah): idxSorted as the sort left it (idxSorted above: as the
    // pass left it), the work list, the boxes per BVH2 node and per sorted primitive
    std::vector<uint32_t> idxMorton;
    std::vector<lbvh::Member> treelets;
    std::vector<float> nbox, pbox;
    // the collapse plan (LbvhGpuBuild::plan): the nodes above the treelets, the packed picks
    // per BVH2 node, the eight costs per node index (set at treelet roots and upper nodes)
    std::vector<lbvh::Member> upper;
    std::vector<uint32_t> picks;
    std::vector<float> pcost;
    std::vector<uint64_t> keysSorted;
    std::vector<GpuBvh8Node> nodes;
    std::vector<GpuTriangle> tris;                // the rows, then the padding record
    std::vector<uint32_t> perm, order, levelOffsets;
    int32_t roots[3] { -1, -1, -1 };
    uint32_t opaqueNodes = 0, depth = 0;
    float inflateAbs = 0.0f;
    bool built = false;
    std::string why;                              // the fallback reason
};

hipError_t buildLbvhGpu(LbvhGpuBuild& g, hipStream_t s, std::string& why)
{
    // Scratch in two allocations (one sized from the snapshot, one from the count of
    // triangles read back): a free waits for the device's streams, frames in flight included
    struct Arena {
        DeviceBuffer buf;
        size_t used = 0;
        static size_t pad(size_t n) { return (n + 255) & ~static_cast<size_t>(255); }
        DeviceBuffer take(size_t n)
        {
            DeviceBuffer b;
            b.ptr = static_cast<char*>(buf.ptr) + used;
            b.bytes = n;
            used += pad(n);
            return b; // a view: never released
        }
        ~Arena() { buf.release(); }
    } arenaA, arenaB;
    struct {
        DeviceBuffer classOf, hdr, idx, idxSorted, keys, keysSorted, sortTemp, split, position, items[2], nodes, counters, masks, inst, boxes, treelets, nbox, pbox, upper, picks, pcost;
    } w;
    hipError_t e = hipSuccess;
    struct KeepWhy {
        LbvhGpuTrace* trace;
        const std::string& why;
        ~KeepWhy()
        {
            if (trace) trace->why = why;
        }
    } keepWhy { g.trace, why };
#define ARK_GB(expr)                          \
    do {                                      \
        if ((e = (expr)) != hipSuccess) return e; \
    } while (0)
    if (g.records == 0 || g.classHost.empty()) {
        why = "no records";
        return hipSuccess;
    }
    const uint32_t records = g.records, instances = static_cast<uint32_t>(g.classHost.size());
    const GpuTriangle* snap = g.snap;
    const std::vector<uint32_t>& classHost = g.classHost;
    ARK_GB(arenaA.buf.alloc(Arena::pad(instances * 4ull) + Arena::pad(sizeof(LbvhHeader)) + Arena::pad(records * 4ull) + Arena::pad(records * 8ull)));
    w.classOf = arenaA.take(instances * 4ull);
    w.hdr = arenaA.take(sizeof(LbvhHeader));
    w.idx = arenaA.take(records * 4ull);
    w.keys = arenaA.take(records * 8ull);
    ARK_GB(hipMemcpyAsync(w.classOf.ptr, classHost.data(), instances * 4ull, hipMemcpyHostToDevice, s));
    ARK_GB(hipStreamWaitEvent(s, g.evSnap, 0));
    if (g.light) {
        LbvhFrame fr;
        std::memcpy(fr.m, g.frame, sizeof(fr.m));
        ARK_GB(launch_lbvh_prims_light(snap, records, instances, fr, g.wBits, w.idx.as<uint32_t>(), w.keys.as<uint64_t>(), w.hdr.as<LbvhHeader>(), s));
    } else {
        ARK_GB(launch_lbvh_prims(snap, records, w.classOf.as<uint32_t>(), instances, w.idx.as<uint32_t>(), w.keys.as<uint64_t>(), w.hdr.as<LbvhHeader>(), s));
    }
    LbvhHeader hdr {};
    ARK_GB(hipMemcpyAsync(&hdr, w.hdr.ptr, sizeof(hdr), hipMemcpyDeviceToHost, s));
    ARK_GB(hipStreamSynchronize(s));
    if (g.light && !hdr.error) hdr.classCount[0] = hdr.prims; // one range [0, n): the keys' class bits are 0
    if (g.trace) g.trace->hdr = hdr;
    if (hdr.error || hdr.prims == 0 || hdr.prims > records || hdr.classCount[0] + hdr.classCount[1] + hdr.classCount[2] != hdr.prims) {
        why = hdr.error ? "record of an unknown instance" : "no triangles";
        return hipSuccess;
    }
    const uint32_t n = hdr.prims;
    // sort the (key, record index) pairs
    size_t tempBytes = 0;
    ARK_GB(launch_lbvh_sort(nullptr, tempBytes, w.keys.as<uint64_t>(), nullptr, w.idx.as<uint32_t>(), nullptr, n, s));
    // (the collapse's bound on the nodes: below)
    const uint32_t nodeCap = n / 2u + 8u;
    // (the SAH pass: treelets are disjoint ranges of at least 4 primitives; its list and boxes live in the same arena)
    // (the collapse plan: treelets of at least 2, fewer than n nodes above them; a word and eight costs per node index)
    const bool plan = g.sah && g.plan;
    const uint32_t treeletCap = plan ? n / 2u + 1u : g.sah ? n / 4u + 1u : 0u;
    const uint32_t upperCap = plan ? n : 0u;
    const size_t sahBoxBytes = g.sah ? n * 6ull * sizeof(float) : 0;
    const size_t picksBytes = plan ? n * 4ull : 0, pcostBytes = plan ? n * 8ull * sizeof(float) : 0;
    {
        const size_t sizes[] = { tempBytes, n * 8ull, n * 4ull, n * 4ull, nodeCap * sizeof(GpuBvh8Node), nodeCap * sizeof(lbvh::Member), nodeCap * sizeof(lbvh::Member),
                                 n * 4ull, kLbvhCounters * 4ull, nodeCap * 8ull, instances * sizeof(RefitInstance), nodeCap * 6ull * sizeof(float),
                                 treeletCap * sizeof(lbvh::Member), sahBoxBytes, sahBoxBytes, upperCap * sizeof(lbvh::Member), picksBytes, pcostBytes };
        size_t total = 0;
        for (size_t b : sizes) total += Arena::pad(b);
        ARK_GB(arenaB.buf.alloc(total));
        w.sortTemp = arenaB.take(sizes[0]);
        w.keysSorted = arenaB.take(sizes[1]);
        w.idxSorted = arenaB.take(sizes[2]);
        w.split = arenaB.take(sizes[3]);
        w.nodes = arenaB.take(sizes[4]);
        w.items[0] = arenaB.take(sizes[5]);
        w.items[1] = arenaB.take(sizes[6]);
        w.position = arenaB.take(sizes[7]);
        w.counters = arenaB.take(sizes[8]);
        w.masks = arenaB.take(sizes[9]);
        w.inst = arenaB.take(sizes[10]);
        w.boxes = arenaB.take(sizes[11]);
        w.treelets = arenaB.take(sizes[12]);
        w.nbox = arenaB.take(sizes[13]);
        w.pbox = arenaB.take(sizes[14]);
        w.upper = arenaB.take(sizes[15]);
        w.picks = arenaB.take(sizes[16]);
        w.pcost = arenaB.take(sizes[17]);
    }
    ARK_GB(launch_lbvh_sort(w.sortTemp.ptr, tempBytes, w.keys.as<uint64_t>(), w.keysSorted.as<uint64_t>(), w.idx.as<uint32_t>(), w.idxSorted.as<uint32_t>(), n, s));
    // the radix trees, class by class
    ARK_GB(hipMemsetAsync(w.counters.ptr, 0, kLbvhCounters * 4, s));
    uint32_t classLo[3], first = 0;
    for (int c = 0; c < 3; ++c) {
        classLo[c] = first;
        first += hdr.classCount[c];
        ARK_GB(launch_lbvh_hierarchy(w.keysSorted.as<uint64_t>(), classLo[c], classLo[c] + hdr.classCount[c], w.split.as<uint32_t>(), s,
                                     g.sah ? w.treelets.as<lbvh::Member>() : nullptr, treeletCap, w.counters.as<uint32_t>(),
                                     plan ? w.upper.as<lbvh::Member>() : nullptr, upperCap));
    }
    uint32_t treelets = 0, upperNodes = 0;
    if (g.sah) {
        // the SAH pass: one workgroup per treelet, the launch sized by the list's count read back
        uint32_t counted[kLbvhCounters] = {};
        if (g.trace) {
            g.trace->idxMorton.resize(n);
            ARK_GB(hipMemcpyAsync(g.trace->idxMorton.data(), w.idxSorted.ptr, n * 4ull, hipMemcpyDeviceToHost, s));
        }
        ARK_GB(hipMemsetAsync(w.nbox.ptr, 0, sahBoxBytes, s));
        ARK_GB(hipMemsetAsync(w.pbox.ptr, 0, sahBoxBytes, s));
        if (plan) {
            ARK_GB(hipMemsetAsync(w.picks.ptr, 0, picksBytes, s));
            ARK_GB(hipMemsetAsync(w.pcost.ptr, 0, pcostBytes, s));
        }
        ARK_GB(hipMemcpyAsync(counted, w.counters.ptr, sizeof(counted), hipMemcpyDeviceToHost, s));
        ARK_GB(hipStreamSynchronize(s));
        treelets = counted[kLbvhTreelets];
        upperNodes = counted[kLbvhUpper];
        if (counted[kLbvhOverflow] || treelets > treeletCap || upperNodes > upperCap) {
            why = "more nodes than the device build's scratch";
            return hipSuccess;
        }
        LbvhTreeletArgs ta {};
        ta.snap = snap;
        ta.list = w.treelets.as<lbvh::Member>();
        ta.prims = n;
        ta.sorted = w.idxSorted.as<uint32_t>();
        ta.split = w.split.as<uint32_t>();
        ta.nbox = w.nbox.as<float>();
        ta.pbox = w.pbox.as<float>();
        ta.light = g.light ? 1 : 0;
        std::memcpy(ta.frame.m, g.frame, sizeof(ta.frame.m));
        ta.picks = plan ? w.picks.as<uint32_t>() : nullptr;
        ta.pcost = plan ? w.pcost.as<float>() : nullptr;
        ARK_GB(launch_lbvh_treelet_sah(ta, treelets, s, plan));
        if (plan) {
            // the nodes above the treelets, behind the treelets' kernel: one workgroup, in rounds
            LbvhUpperArgs ua {};
            ua.snap = snap;
            ua.list = w.upper.as<lbvh::Member>();
            ua.count = upperNodes;
            ua.prims = n;
            ua.sorted = w.idxSorted.as<uint32_t>();
            ua.split = w.split.as<uint32_t>();
            ua.nbox = w.nbox.as<float>();
            ua.pbox = w.pbox.as<float>();
            ua.picks = w.picks.as<uint32_t>();
            ua.pcost = w.pcost.as<float>();
            ua.counters = w.counters.as<uint32_t>();
            ua.light = ta.light;
            ua.frame = ta.frame;
            ARK_GB(launch_lbvh_upper_plan(ua, s));
        }
    }
    // the collapse. Every BVH8 node but a class's root is a BVH2 node of at least 4
    // triangles, and one with an internal child has 8 members. With L nodes without an
    // internal child (4 triangles of their own each), C with one (7 members of their
    // own) and fewer than L with more, 4 L + 7 C <= n bounds 2 L + C by n / 2: fewer than
    // n / 2 + 3 nodes (the kernel checks, and the job falls back beyond).
    float lo[3], hi[3];
    LbvhCollapseArgs a {};
    for (int k = 0; k < 3; ++k) {
        lo[k] = lbvhOrderedFloat(hdr.lo[k]);
        hi[k] = lbvhOrderedFloat(hdr.hi[k]);
        a.extent[k] = hi[k] - lo[k];
    }
    a.keys = w.keysSorted.as<uint64_t>();
    a.split = w.split.as<uint32_t>();
    a.nodes = w.nodes.as<GpuBvh8Node>();
    a.position = w.position.as<uint32_t>();
    a.counters = w.counters.as<uint32_t>();
    a.criterion = g.sah ? lbvh::kOpenLargestBox : lbvh::kDefaultCriterion;
    a.slotRule = g.slotRule;
    a.wBits = g.wBits;
    a.useSah = g.sah ? 1 : 0;
    a.sah.nbox = w.nbox.as<float>();
    a.sah.pbox = w.pbox.as<float>();
    for (int k = 0; k < 3; ++k) {
        a.sah.lo[k] = lo[k];
        a.sah.hi[k] = hi[k];
    }
    std::vector<std::array<uint32_t, 3>> levels; // node counts [depth][class]
    uint32_t nodeTotal = 0, counters[kLbvhCounters] = {};
    for (int c = 0; c < 3; ++c) {
        if (!hdr.classCount[c]) continue;
        g.roots[c] = static_cast<int32_t>(nodeTotal);
        a.items = nullptr;
        a.root.r.first = classLo[c];
        a.root.r.last = classLo[c] + hdr.classCount[c] - 1u;
        a.root.node = classLo[c];
        a.count = 1;
        a.levelBase = nodeTotal;
        int pong = 0;
        for (uint32_t depth = 0; a.count; ++depth) {
            if (depth >= kGpuBuildMaxDepth || a.levelBase + a.count > nodeCap) {
                why = depth >= kGpuBuildMaxDepth ? "BVH8 deeper than the device build installs" : "more nodes than the device build's scratch";
                return hipSuccess;
            }
            a.nextBase = a.levelBase + a.count;
            a.nextCapacity = nodeCap - a.nextBase;
            a.next = w.items[pong].as<lbvh::Member>();
            ARK_GB(hipMemsetAsync(w.counters.as<uint32_t>() + kLbvhNextCount, 0, 4, s));
            ARK_GB(launch_lbvh_collapse(a, s, plan ? w.picks.as<uint32_t>() : nullptr));
            // the level's count, before the next level is launched
            ARK_GB(hipMemcpyAsync(counters, w.counters.ptr, sizeof(counters), hipMemcpyDeviceToHost, s));
            ARK_GB(hipStreamSynchronize(s));
            if (counters[kLbvhOverflow]) {
                why = "more nodes than the device build's scratch";
                return hipSuccess;
            }
            if (counters[kLbvhPlanStalled]) {
                why = "the collapse plan did not finish";
                return hipSuccess;
            }
            if (levels.size() <= depth) levels.push_back({ 0u, 0u, 0u });
            levels[depth][c] = a.count;
            a.items = a.next;
            a.levelBase = a.nextBase;
            a.count = counters[kLbvhNextCount];
            pong ^= 1;
        }
        nodeTotal = a.levelBase;
        if (c == 0) g.opaqueNodes = nodeTotal;
        if (c == 0) g.opaqueRecords = counters[kLbvhRecords]; // (the classes' leaf rows follow one another)
    }
    const uint32_t outRecords = counters[kLbvhRecords];
    if (!(DeviceBvh::bytesFor(nodeTotal, outRecords) < (1ull << 32))) {
        why = "nodes and records of 4 GiB or more";
        return hipSuccess;
    }
    // the installed buffers, sized from the counts read back
    DeviceBvh& b = *g.bvh;
    b.triOffset = DeviceBvh::triOffsetFor(nodeTotal);
    ARK_GB(b.buf.alloc(DeviceBvh::bytesFor(nodeTotal, outRecords)));
    if (g.perm) ARK_GB(g.perm->alloc(std::max<size_t>(16, outRecords * 4ull)));
    GpuBvh8Node* nodes = b.nodes(b.buf);
    GpuTriangle* tris = b.tris(b.buf);
    ARK_GB(hipMemcpyAsync(nodes, w.nodes.ptr, nodeTotal * sizeof(GpuBvh8Node), hipMemcpyDeviceToDevice, s));
    ARK_GB(launch_lbvh_scatter(snap, w.idxSorted.as<uint32_t>(), w.position.as<uint32_t>(), tris, g.perm ? g.perm->as<uint32_t>() : nullptr, n, outRecords, s));
    // the refit's level order from the level counts (bvhLevelOrder's format: deepest level
    // first, ascending node index within a level; each class one breadth-first range)
    std::vector<uint32_t>& order = g.order;
    order.clear();
    order.reserve(nodeTotal);
    b.levelOffsets.assign(1, 0u);
    {
        std::vector<std::array<uint32_t, 3>> base(levels.size());
        uint32_t at[3];
        for (int c = 0; c < 3; ++c) at[c] = g.roots[c] >= 0 ? static_cast<uint32_t>(g.roots[c]) : 0u;
        for (size_t d = 0; d < levels.size(); ++d)
            for (int c = 0; c < 3; ++c) {
                base[d][c] = at[c];
                at[c] += levels[d][c];
            }
        for (size_t d = levels.size(); d-- > 0;) {
            for (int c = 0; c < 3; ++c)
                for (uint32_t k = 0; k < levels[d][c]; ++k) order.push_back(base[d][c] + k);
            b.levelOffsets.push_back(static_cast<uint32_t>(order.size()));
        }
    }
    ARK_GB(b.order.alloc(std::max<size_t>(16, order.size() * 4)));
    ARK_GB(hipMemcpyAsync(b.order.ptr, order.data(), order.size() * 4, hipMemcpyHostToDevice, s));
    // boxes, grids and planes: the refit over every level, deepest first, every node live
    // (all mask bits set, no instance dirty: no record is touched), the inflation hostBuildWorld's
    // or, in light coordinates, build_sun_bvh's (the box and the largest |coordinate| are
    // min / max reductions: the same bits whatever the order)
    ARK_GB(hipMemsetAsync(w.masks.ptr, 0xff, nodeTotal * 8ull, s));
    ARK_GB(hipMemsetAsync(w.inst.ptr, 0, instances * sizeof(RefitInstance), s));
    RefitBoxArgs ra {};
    ra.inflate = bvh8_inflation_box(lo, hi);
    ra.light = 0;
    if (g.light) {
        float maxAbs;
        std::memcpy(&maxAbs, &hdr.maxAbs, 4);
        ra.inflate = 2.0f * bvh8_inflation_box(lo, hi) + 2e-6f * maxAbs;
        ra.light = 1;
        std::memcpy(ra.frame, g.frame, sizeof(ra.frame));
    }
    g.inflateAbs = ra.inflate;
    ra.dirty = ~0ull;
    for (size_t l = 0; l + 1 < b.levelOffsets.size(); ++l)
        ARK_GB(launch_refit_nodes(nodes, tris, w.boxes.as<float>(), b.order.as<uint32_t>() + b.levelOffsets[l], b.levelOffsets[l + 1] - b.levelOffsets[l], ra,
                                  w.masks.as<uint64_t>(), w.inst.as<RefitInstance>(), nullptr, nullptr, s));
    ARK_GB(hipStreamSynchronize(s));
    if (LbvhGpuTrace* t = g.trace) {
        t->idx.resize(n);
        t->idxSorted.resize(n);
        t->split.resize(n);
        t->keysSorted.resize(n);
        t->nodes.resize(nodeTotal);
        t->tris.resize(outRecords + 1ull);
        t->perm.resize(g.perm ? outRecords : 0u);
        ARK_GB(hipMemcpyAsync(t->idx.data(), w.idx.ptr, n * 4ull, hipMemcpyDeviceToHost, s));
        ARK_GB(hipMemcpyAsync(t->idxSorted.data(), w.idxSorted.ptr, n * 4ull, hipMemcpyDeviceToHost, s));
        ARK_GB(hipMemcpyAsync(t->split.data(), w.split.ptr, n * 4ull, hipMemcpyDeviceToHost, s));
        ARK_GB(hipMemcpyAsync(t->keysSorted.data(), w.keysSorted.ptr, n * 8ull, hipMemcpyDeviceToHost, s));
        ARK_GB(hipMemcpyAsync(t->nodes.data(), nodes, nodeTotal * sizeof(GpuBvh8Node), hipMemcpyDeviceToHost, s));
        ARK_GB(hipMemcpyAsync(t->tris.data(), tris, (outRecords + 1ull) * sizeof(GpuTriangle), hipMemcpyDeviceToHost, s));
        if (!t->perm.empty()) ARK_GB(hipMemcpyAsync(t->perm.data(), g.perm->ptr, outRecords * 4ull, hipMemcpyDeviceToHost, s));
        if (g.sah) {
            t->treelets.resize(treelets);
            t->nbox.resize(n * 6ull);
            t->pbox.resize(n * 6ull);
            if (treelets) ARK_GB(hipMemcpyAsync(t->treelets.data(), w.treelets.ptr, treelets * sizeof(lbvh::Member), hipMemcpyDeviceToHost, s));
            ARK_GB(hipMemcpyAsync(t->nbox.data(), w.nbox.ptr, sahBoxBytes, hipMemcpyDeviceToHost, s));
            ARK_GB(hipMemcpyAsync(t->pbox.data(), w.pbox.ptr, sahBoxBytes, hipMemcpyDeviceToHost, s));
        }
        if (plan) {
            t->upper.resize(upperNodes);
            t->picks.resize(n);
            t->pcost.resize(n * 8ull);
            if (upperNodes) ARK_GB(hipMemcpyAsync(t->upper.data(), w.upper.ptr, upperNodes * sizeof(lbvh::Member), hipMemcpyDeviceToHost, s));
            ARK_GB(hipMemcpyAsync(t->picks.data(), w.picks.ptr, picksBytes, hipMemcpyDeviceToHost, s));
            ARK_GB(hipMemcpyAsync(t->pcost.data(), w.pcost.ptr, pcostBytes, hipMemcpyDeviceToHost, s));
        }
        ARK_GB(hipStreamSynchronize(s));
        t->order = order;
        t->levelOffsets = b.levelOffsets;
        std::copy(g.roots, g.roots + 3, t->roots);
        t->opaqueNodes = g.opaqueNodes;
        t->depth = static_cast<uint32_t>(levels.size());
        t->inflateAbs = ra.inflate;
        t->built = true;
    }
#undef ARK_GB
    b.nodeCount = nodeTotal;
    b.records = outRecords;
    b.depth = static_cast<uint32_t>(levels.size());
    g.prims = n;
    return hipSuccess;
}

} // namespace ark

// ark_ddgi_debug.h: one traced device build (buildLbvhGpu, the product's kernels and
// nothing else) of the given records on a stream of its own, without a context, against
// build_lbvh_host of the same records in the device's compaction order, stage by stage.
namespace {
// out: 48 words (ark_ddgi_debug_lbvh_device_parity_plan's)
int lbvhDeviceParity(int device, const void* records, uint64_t n_records, const int32_t* class_of, uint32_t n_instances, const float* sun_dir, int w_bits, bool sahPass,
                     bool planPass, uint64_t* out)
{
    planPass = planPass && sahPass;
    using namespace ark;
    if (!records || !class_of || !out || n_records == 0 || n_records > 0x7fffffffull || n_instances == 0) return -1;
    std::fill(out, out + 48, uint64_t(0));
    for (uint32_t i = 0; i < n_instances; ++i)
        if (class_of[i] < 0 || class_of[i] > 2) return -1; // (the kernels index the class counts by it)
    int wBits = lbvh::kMortonBits;
    if (sun_dir) {
        wBits = w_bits < 0 ? lbvh::kSunKeyBitsW : w_bits;
        if (wBits > lbvh::kMortonBits || (wBits & 1)) return -1;
    }
    const uint32_t n = static_cast<uint32_t>(n_records);
    std::vector<GpuTriangle> rec(n);
    std::memcpy(rec.data(), records, n * sizeof(GpuTriangle));

    // the device build
    struct Device {
        hipStream_t s = nullptr;
        hipEvent_t ev = nullptr;
        DeviceBuffer snap, perm;
        DeviceBvh bvh;
        ~Device()
        {
            if (s) (void)hipStreamSynchronize(s);
            bvh.release();
            perm.release();
            snap.release();
            if (ev) (void)hipEventDestroy(ev);
            if (s) (void)hipStreamDestroy(s);
        }
    } d;
    LbvhGpuTrace trace;
    LbvhGpuBuild g;
    std::string why;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&d.s, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&d.ev, hipEventDisableTiming);
    if (e == hipSuccess) e = d.snap.alloc(std::max<size_t>(16, n * sizeof(GpuTriangle)));
    if (e == hipSuccess) e = hipMemcpyAsync(d.snap.ptr, rec.data(), n * sizeof(GpuTriangle), hipMemcpyHostToDevice, d.s);
    if (e == hipSuccess) e = hipEventRecord(d.ev, d.s);
    if (e == hipSuccess) {
        g.snap = d.snap.as<GpuTriangle>();
        g.evSnap = d.ev;
        g.records = n;
        g.classHost.assign(class_of, class_of + n_instances);
        if (sun_dir) {
            double frame[3][3];
            sun_frame(sun_dir, frame);
            g.light = true;
            std::memcpy(g.frame, frame, sizeof(g.frame));
            g.slotRule = lbvh::kSlotsAscendingW;
            g.wBits = wBits;
        }
        g.bvh = &d.bvh;
        g.perm = &d.perm;
        g.trace = &trace;
        g.sah = sahPass;
        g.plan = planPass;
        e = buildLbvhGpu(g, d.s, why);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(d.s);
    out[26] = static_cast<uint64_t>(e);
    if (e != hipSuccess) return -5;
    static const char* const kWhy[] = { "", "no records", "no triangles", "record of an unknown instance", "BVH8 deeper than the device build installs",
                                        "more nodes than the device build's scratch", "nodes and records of 4 GiB or more" }; // (another, the plan's included: 7)
    out[4] = 7;
    for (uint64_t k = 0; k < sizeof(kWhy) / sizeof(kWhy[0]); ++k)
        if (trace.why == kWhy[k]) out[4] = k;
    out[0] = trace.hdr.prims;
    if (!trace.why.empty() || !trace.built) return 2; // the host's scene: nothing was built

    // the compaction: a permutation of exactly the records that are not holes
    std::vector<uint32_t> live;
    for (uint32_t i = 0; i < n; ++i)
        if (!isHoleTriangle(rec[i])) live.push_back(i);
    {
        std::vector<uint32_t> sorted = trace.idx;
        std::sort(sorted.begin(), sorted.end());
        out[5] = sorted.size() != live.size() ? 1u : 0u;
        for (size_t j = 0; j < std::min(sorted.size(), live.size()); ++j) out[5] += sorted[j] != live[j] ? 1u : 0u;
    }
    if (sun_dir && !out[5] && !live.empty()) {
        // k_lbvh_prims_light: a wave's survivors one run, ascending
        uint64_t runs = 1, waves = 1;
        for (size_t j = 0; j + 1 < trace.idx.size(); ++j) {
            if ((trace.idx[j] >> 6) != (trace.idx[j + 1] >> 6)) runs++;
            else if (trace.idx[j] >= trace.idx[j + 1]) out[6]++;
            if ((live[j] >> 6) != (live[j + 1] >> 6)) waves++;
        }
        if (runs != waves) out[6]++;
    }
    std::vector<int> classOf(class_of, class_of + n_instances);
    LbvhSunOptions so;
    std::memcpy(so.frame, g.frame, sizeof(so.frame));
    so.wBits = wBits;
    const LbvhHostResult r = build_lbvh_host(rec, classOf, lbvh::kDefaultCriterion, sun_dir ? &so : nullptr, out[5] ? nullptr : &trace.idx, sahPass, planPass);
    auto bits = [](float f) {
        uint32_t u;
        std::memcpy(&u, &f, 4);
        return u;
    };
    // the header
    const uint32_t prims = static_cast<uint32_t>(live.size());
    out[7] = (trace.hdr.prims != prims ? 1u : 0u) + (trace.hdr.error ? 1u : 0u);
    for (int c = 0; c < 3; ++c) out[7] += trace.hdr.classCount[c] != r.classCount[c] ? 1u : 0u;
    for (int k = 0; k < 3; ++k) {
        // (== of floats: the ordered-bits atomics tell -0 from +0, std::min does not, and nothing later depends on a zero's sign)
        out[8] += lbvhOrderedFloat(trace.hdr.lo[k]) == r.sceneLo[k] ? 0u : 1u;
        out[8] += lbvhOrderedFloat(trace.hdr.hi[k]) == r.sceneHi[k] ? 0u : 1u;
    }
    out[9] = trace.hdr.maxAbs != bits(r.maxAbs) ? 1u : 0u;
    out[10] = bits(trace.inflateAbs) != bits(r.inflateAbs) ? 1u : 0u;
    // keys, sorted records, splits
    if (trace.keysSorted.size() != prims || trace.idxSorted.size() != prims || trace.split.size() != prims || r.keysSorted.size() != prims) {
        out[11] = out[12] = out[13] = 1;
    } else {
        for (uint32_t j = 0; j < prims; ++j) {
            out[11] += trace.keysSorted[j] != r.keysSorted[j] ? 1u : 0u;
            // (the SAH pass: [12] the order the sort left, [31] the order the pass left)
            const std::vector<uint32_t>& dm = sahPass ? trace.idxMorton : trace.idxSorted;
            const std::vector<uint32_t>& hm = sahPass ? r.idxMorton : r.idxSorted;
            out[12] += j >= dm.size() || j >= hm.size() || dm[j] != hm[j] ? 1u : 0u;
            if (sahPass) out[31] += trace.idxSorted[j] != r.idxSorted[j] ? 1u : 0u;
        }
        uint32_t first = 0;
        for (int c = 0; c < 3; ++c) {
            for (uint32_t i = first; i + 1u < first + r.classCount[c]; ++i) out[13] += trace.split[i] != r.split[i] ? 1u : 0u;
            first += r.classCount[c];
        }
    }
    if (sahPass) {
        // the work list as a set, the boxes by bits
        auto less = [](const lbvh::Member& a, const lbvh::Member& b) { return a.r.first < b.r.first; };
        std::vector<lbvh::Member> dl = trace.treelets, hl = r.treelets;
        std::sort(dl.begin(), dl.end(), less);
        std::sort(hl.begin(), hl.end(), less);
        out[29] = dl.size();
        out[30] = dl.size() != hl.size() ? 1u : 0u;
        for (size_t k = 0; k < std::min(dl.size(), hl.size()); ++k)
            out[30] += dl[k].r.first != hl[k].r.first || dl[k].r.last != hl[k].r.last || dl[k].node != hl[k].node ? 1u : 0u;
        out[32] = trace.nbox.size() != r.nbox.size() ? 1u : 0u;
        out[33] = trace.pbox.size() != r.pbox.size() ? 1u : 0u;
        for (size_t k = 0; k < std::min(trace.nbox.size(), r.nbox.size()); ++k) out[32] += bits(trace.nbox[k]) != bits(r.nbox[k]) ? 1u : 0u;
        for (size_t k = 0; k < std::min(trace.pbox.size(), r.pbox.size()); ++k) out[33] += bits(trace.pbox[k]) != bits(r.pbox[k]) ? 1u : 0u;
    }
    if (planPass) {
        // the upper list as a set; the picks at every node index, the costs of the treelet
        // roots and upper nodes (all else 0 on both sides) and the upper nodes' boxes, by bits
        auto less = [](const lbvh::Member& a, const lbvh::Member& b) { return a.node < b.node; };
        std::vector<lbvh::Member> dl = trace.upper, hl = r.upper;
        std::sort(dl.begin(), dl.end(), less);
        std::sort(hl.begin(), hl.end(), less);
        out[34] = dl.size();
        out[38] = dl.size() != hl.size() ? 1u : 0u;
        for (size_t k = 0; k < std::min(dl.size(), hl.size()); ++k)
            out[38] += dl[k].r.first != hl[k].r.first || dl[k].r.last != hl[k].r.last || dl[k].node != hl[k].node ? 1u : 0u;
        out[35] = trace.picks.size() != r.picks.size() ? 1u : 0u;
        for (size_t k = 0; k < std::min(trace.picks.size(), r.picks.size()); ++k) out[35] += trace.picks[k] != r.picks[k] ? 1u : 0u;
        out[36] = trace.pcost.size() != r.pcost.size() ? 1u : 0u;
        for (size_t k = 0; k < std::min(trace.pcost.size(), r.pcost.size()); ++k) out[36] += bits(trace.pcost[k]) != bits(r.pcost[k]) ? 1u : 0u;
        for (const lbvh::Member& m : hl)
            for (int q = 0; q < 6; ++q) {
                const size_t at = 6ull * m.node + static_cast<size_t>(q);
                out[37] += at >= trace.nbox.size() || at >= r.nbox.size() || bits(trace.nbox[at]) != bits(r.nbox[at]) ? 1u : 0u;
            }
        out[39] = r.planRounds;
        if (r.planStalled) out[35]++;
    }
    // the tree
    const GpuTriangle padding = trace.tris.back(); // (records + 1 entries)
    trace.tris.pop_back();
    Bvh8TreeView dv, hv;
    dv.nodes = &trace.nodes;
    dv.tris = &trace.tris;
    dv.perm = &trace.perm;
    dv.order = &trace.order;
    dv.levelOffsets = &trace.levelOffsets;
    dv.padding = &padding;
    std::copy(trace.roots, trace.roots + 3, dv.roots);
    dv.opaqueNodes = trace.opaqueNodes;
    dv.depth = trace.depth;
    hv.nodes = &r.nodes;
    hv.tris = &r.tris;
    hv.perm = &r.perm;
    hv.order = &r.order;
    hv.levelOffsets = &r.levelOffsets;
    std::copy(r.roots, r.roots + 3, hv.roots);
    hv.opaqueNodes = r.opaqueNodes;
    hv.depth = r.depth;
    const Bvh8CanonicalDiff diff = compare_bvh8_canonical(dv, hv);
    out[1] = trace.nodes.size();
    out[2] = trace.tris.size();
    out[3] = trace.depth;
    out[14] = diff.shape;
    out[15] = diff.header;
    out[16] = diff.grid;
    out[17] = diff.planes;
    out[18] = diff.children;
    out[19] = diff.records;
    out[20] = diff.perm;
    out[21] = diff.holes;
    out[22] = diff.levelOrder;
    out[23] = diff.padding;
    out[24] = static_cast<uint64_t>(diff.firstA);
    out[25] = static_cast<uint64_t>(diff.firstB);
    out[27] = diff.pairs;
    out[28] = r.nodes.size();
    uint64_t mismatches = 0;
    for (int k = 5; k <= 23; ++k) mismatches += out[k];
    mismatches += out[30] + out[31] + out[32] + out[33] + out[35] + out[36] + out[37] + out[38];
    return mismatches ? 1 : 0;
}
} // namespace

extern "C" int ark_ddgi_debug_lbvh_device_parity(int device, const void* records, uint64_t n_records, const int32_t* class_of, uint32_t n_instances,
                                                  const float* sun_dir, int w_bits, uint64_t* out)
{
    if (!records || !class_of || !out || n_records == 0 || n_records > 0x7fffffffull || n_instances == 0) return -1;
    uint64_t all[48];
    const int rc = lbvhDeviceParity(device, records, n_records, class_of, n_instances, sun_dir, w_bits, false, false, all);
    std::copy(all, all + 32, out);
    return rc;
}

extern "C" int ark_ddgi_debug_lbvh_device_parity_sah(int device, const void* records, uint64_t n_records, const int32_t* class_of, uint32_t n_instances,
                                                      const float* sun_dir, int w_bits, int sah, uint64_t* out)
{
    if (!records || !class_of || !out || n_records == 0 || n_records > 0x7fffffffull || n_instances == 0) return -1;
    uint64_t all[48];
    const int rc = lbvhDeviceParity(device, records, n_records, class_of, n_instances, sun_dir, w_bits, sah != 0, false, all);
    std::copy(all, all + 40, out);
    return rc;
}

extern "C" int ark_ddgi_debug_lbvh_device_parity_plan(int device, const void* records, uint64_t n_records, const int32_t* class_of, uint32_t n_instances,
                                                       const float* sun_dir, int w_bits, int sah, int plan, uint64_t* out)
{
    return lbvhDeviceParity(device, records, n_records, class_of, n_instances, sun_dir, w_bits, sah != 0, plan != 0, out);
}
