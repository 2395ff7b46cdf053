// Buffer handles and who holds them.  The reference frees and reuses buffer storage and queue items (core/buffer_storage.h:47-77,
// core/voice.h:84-98): a host that deletes a buffer gives its handle up, and the handle dies once its last holder lets go.
#include "buffer_table.hpp"
#include <algorithm>

namespace oalgpu {

void BufferTable::reset(uint32_t places, uint32_t voices)
{
    mRecs.assign(std::max(places, 1u), BufferRecord{});
    mPlaces = places; mUsed = 0;
    mFree.clear();
    mHead.assign(std::max(voices, 1u), -1);
    mDoneKnown.assign(mHead.size(), 0u);
    mUnqueued.assign(mHead.size(), 0u);
}

int BufferTable::alloc(void *storage, uint32_t loopLen, int parent)
{
    uint32_t h;
    if(!mFree.empty()) { h = mFree.back(); mFree.pop_back(); }
    else if(mUsed < mPlaces) h = mUsed++;
    else return -1;
    mRecs[h] = BufferRecord{true, false, parent < 0 ? -1 : parent, -1, 0u, storage, loopLen};
    if(parent >= 0) ++mRecs[size_t(parent)].refs;
    return int(h);
}

// `h` dies if it is released and unheld -- with letGo, after one holder of it has let go.  A handle that dies lets go of its
// parent and then of its queue link, which may die in turn: they wait on a stack (the parent on top), so a queue of any
// length dies in queue order without recursion.
FreedStorage BufferTable::reap(int h, bool letGo)
{
    FreedStorage freed;
    for(std::vector<int32_t> work{h}; !work.empty(); letGo = true)
    {
        const int32_t cur = work.back(); work.pop_back();
        if(cur < 0) continue;
        BufferRecord &b = mRecs[size_t(cur)];
        if(letGo && b.refs) --b.refs;
        if(b.refs != 0 || !b.released || !b.live) continue;
        if(b.storage) freed.push_back(b.storage);
        work.push_back(b.next);
        work.push_back(b.parent);
        b = BufferRecord{};
        mFree.push_back(uint32_t(cur));
    }
    return freed;
}

// a queue link or a voice slot's hold points at another handle (to < 0: at none): the new target is held, the old one let go
FreedStorage BufferTable::retarget(int32_t &ref, int to)
{
    const int32_t old = ref;
    ref = to < 0 ? -1 : to;
    if(to >= 0) ++mRecs[size_t(to)].refs;
    return reap(old, true);
}

FreedStorage BufferTable::unqueue(uint32_t voice, uint32_t count)
{
    int32_t head = mHead[voice];
    for(uint32_t i = 0; i < count && head >= 0; ++i) head = mRecs[size_t(head)].next;
    mUnqueued[voice] += count;
    return retarget(mHead[voice], head);
}

} // namespace oalgpu
