// copy_book.h — the one record of what a scene's three geometry copies hold, and so of
// what a refit must re-derive. Pure host code without a HIP dependency, tested on its own
// (tests/cpp/copy_book_test.cpp). The store reports what happened, one method per event.
// The geometry a refit writes comes in three copies: the front one (what the kernels read)
// and two spares. A refit brings the next spare from the transforms it holds to the new
// ones on the store's refit stream and makes it the front one: it waits only for the
// operations that read that copy while it was the front one, two refits before (the frame
// before last), so that it runs beside the frame in flight's traversal and the next
// traversal does not wait for it (with two copies it waited for the previous frame's
// shading, and the frames ran one after the other: C4 4.3 ms per moving frame, static
// 3.3). An install (a new topology) drops the spares; the next refit copies the front one.
// The boxes scratch (DeviceBvh::boxes) is one for the three copies: after every refit it
// holds, for every node, the box of the latest transforms at DeviceBvh::boxesInflate.
#pragma once

#include <array>
#include <cstring>

#include "vertex_dirty.h"

namespace ark {

struct CopyBook {
    using Xf = std::array<float, 12>;
    enum Refit { Target, Forward }; // of the next spare; an install's of the front copy, every instance
    struct Slot {
        std::vector<Xf> xf;       // the transforms its records were written with
        float infl[2] = { 0, 0 }; // its boxes' inflations (world, sun; 0: set_scene's own, so its first refit reaches every node)
        bool valid = false;       // it holds the front copy's topology (its vertex version: vtx.copy)
    } slot[3];
    std::array<int, 3> order { 0, 1, 2 }; // the slots of the front copy, the next refit's target, the last spare
    std::vector<Xf> last;                 // the transforms of the refit before, whichever copy it wrote
    VertexVersions vtx;                   // the instances' vertex versions, the slots' and the boxes scratch's
    bool full = true; // the next refit reaches every node (a new topology, or a scratch not of this one)

    int front() const { return order[0]; }
    int target() const { return order[1]; }
    bool targetValid() const { return slot[target()].valid; }
    // the held inflation of a slot's boxes (refitBvh reads it and writes the refit's)
    float& inflation(int s, int which) { return slot[s].infl[which]; }

    // set_scene: every slot is of `inst`'s transforms (Inst: object_to_world), only slot 0 exists
    template<class Inst>
    void newScene(const Inst* inst, size_t n)
    {
        *this = CopyBook {};
        set(last, inst, n);
        for (Slot& s : slot) s.xf = last;
        slot[0].valid = true;
    }
    // the target was copied from the front one
    void copied()
    {
        slot[target()] = slot[front()];
        vtx.copied(target(), front());
    }
    // A vertex update touched these instances (one flag each): their vertices are newer than
    // every copy's records from here on, whatever becomes of the call's refit
    void vertexUpdate(const std::vector<uint8_t>& touched)
    {
        vtx.begin(touched.size());
        for (size_t i = 0; i < touched.size(); ++i)
            if (touched[i]) vtx.touch(i);
    }
    // A refit to the transform M of instance i must re-derive its records. Target: M differs
    // from the one the target's records hold, or from the refit before's - which keeps the
    // boxes scratch current: a node is skipped only when nothing below it changed since the
    // scratch last saw it, whichever copy that refit wrote; an instance back at the pose
    // the target holds (a nudge and return, a loop of period 3) is re-transformed to the
    // same bits - or its vertices are newer than either. Forward: a snapshot's records, every one.
    bool dirty(Refit r, size_t i, const float* M) const
    {
        const std::vector<Xf>& have = slot[target()].xf;
        return r == Forward || i >= have.size() || i >= last.size() || std::memcmp(have[i].data(), M, sizeof(Xf)) != 0 || std::memcmp(last[i].data(), M, sizeof(Xf)) != 0 ||
               vtx.dirty(i, target());
    }
    // the target was refitted to `inst`'s transforms: it becomes the front copy, that one the last spare
    template<class Inst>
    void refitted(const Inst* inst, size_t n)
    {
        set(last, inst, n);
        slot[target()].xf = last;
        vtx.refitted(target());
        full = false;
        order = { order[1], order[2], order[0] };
    }
    // a refit or its staging failed: the target may be half written, the scratch too
    void targetUnknown()
    {
        slot[target()].valid = false;
        full = true;
    }
    // the spares' buffers were dropped
    void sparesDropped() { slot[order[1]].valid = slot[order[2]].valid = false; }
    // An install replaced a BVH of the front copy by a build over a snapshot of its records:
    // the spares and the boxes scratch are of the old topology, the front copy is of the latest
    // transforms - by the forward refit that follows (refits came in since the snapshot) or still.
    void installed(bool forwardRefit)
    {
        sparesDropped();
        full = true;
        slot[front()].xf = last;
        vtx.installed(front(), forwardRefit);
    }

private:
    template<class Inst>
    static void set(std::vector<Xf>& xf, const Inst* inst, size_t n)
    {
        xf.resize(n);
        for (size_t i = 0; i < n; ++i) std::memcpy(xf[i].data(), inst[i].object_to_world, sizeof(Xf));
    }
};

} // namespace ark
