// The buffer handles of a context and their lifetime (oalgpu_buffer_release): pure bookkeeping, no HIP.  See buffer_table.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace oalgpu {

// A handle dies -- its storage is freed, and the handle reused -- when the host has released it AND nothing holds it any more:
// no voice slot that was started on it (until the slot is started again or stopped), no live buffer whose queue link points at
// it, no channel view of it.
struct BufferRecord {
    bool live{false}, released{false};
    int32_t parent{-1}, next{-1};          // the buffer a channel view looks into; the queue link
    uint32_t refs{0};
    void *storage{nullptr};                // the caller's: opaque here and never freed here (null: a view)
    uint32_t loopLen{0};                   // loop_end - loop_start (0: cannot loop)
};
// what a call that may let go of a buffer returns: the storage of the handles that died by it, in the order they died.  The
// caller frees it (the device must be through with it by then).
using FreedStorage = std::vector<void*>;

class BufferTable {
public:
    void reset(uint32_t places, uint32_t voices);
    bool full() const { return mFree.empty() && mUsed >= mPlaces; }
    bool inRange(int h) const { return h >= 0 && size_t(h) < mRecs.size(); }     // (a table of no places still answers for handle 0)
    const BufferRecord &at(int h) const { return mRecs[size_t(h)]; }
    bool live(int h) const { return h >= 0 && uint32_t(h) < mUsed && mRecs[size_t(h)].live; }
    bool usable(int h) const { return live(h) && !mRecs[size_t(h)].released; }     // may be named by a start, a link, a view
    int alloc(void *storage, uint32_t loopLen, int parent);    // a freed handle first; holds `parent` (a view); -1: table full
    FreedStorage release(int h) { mRecs[size_t(h)].released = true; return reap(h, false); }   // the host gives a usable handle up
    // the queue link of `h` (next < 0: the queue ends there): the link holds its target
    FreedStorage link(int h, int next) { return retarget(mRecs[size_t(h)].next, next); }
    // voice slots.  A start: the slot holds h, lets go of its old head and counts its queue from 0; a stop: it holds nothing
    bool headReleased(uint32_t voice) const { return mHead[voice] >= 0 && mRecs[size_t(mHead[voice])].released; }
    FreedStorage start(uint32_t voice, int h) { mDoneKnown[voice] = mUnqueued[voice] = 0; return retarget(mHead[voice], h); }
    FreedStorage stop(uint32_t voice) { return retarget(mHead[voice], -1); }
    // streaming voices: the buffers the host has READ BACK as played through, and those it has given up of them
    void noteQueueDone(uint32_t voice, uint32_t done) { mDoneKnown[voice] = done; }
    bool canUnqueue(uint32_t voice, uint32_t count) const { return mUnqueued[voice] + count <= mDoneKnown[voice]; }
    FreedStorage unqueue(uint32_t voice, uint32_t count);      // the slot's hold moves `count` links on
private:
    FreedStorage retarget(int32_t &ref, int to);
    FreedStorage reap(int h, bool letGo);
    std::vector<BufferRecord> mRecs;
    uint32_t mPlaces{0}, mUsed{0};         // mUsed: handles handed out so far (dead ones are reused: mFree)
    std::vector<uint32_t> mFree, mDoneKnown, mUnqueued;
    std::vector<int32_t> mHead;            // [voice] the buffer the slot was started on (a queue: its first), -1: none
};

} // namespace oalgpu
