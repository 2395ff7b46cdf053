// Effect slot targets: the order in which a context's slots are processed.
//
// The reference sorts the slots of a context so that a slot comes in front of the slot it targets (alc/alu.cpp:2220-2249: the
// slots without a target are partitioned to the back, then those that target that group in front of it, and so on), and each
// effect then writes into its target's wet buffer (alu.cpp:627-632).  The groups of that partition are the depths computed
// here: depth 0 has no target, depth d targets a slot of depth d - 1.  Within a group the reference's order is whatever
// std::partition leaves; here it is the slot index, ascending, so that the sums on a shared target are the same every time.
#include "slot_order.hpp"

#include <stddef.h>
#include <vector>

namespace oalgpu {

bool SlotOrder(const int32_t *targets, uint32_t numSlots, uint32_t *order, uint32_t *depth)
{
    if(numSlots == 0) return true;
    if(!targets || !order) return false;
    for(uint32_t i = 0; i < numSlots; ++i)
        if(targets[i] < -1 || targets[i] >= int64_t{numSlots} || targets[i] == int64_t{i}) return false;

    // every chain is walked once: up to the first slot whose depth is known (or that has no target), then back down
    constexpr uint32_t kUnknown = 0xffffffffu, kOnPath = 0xfffffffeu;
    std::vector<uint32_t> d(numSlots, kUnknown), path;
    for(uint32_t i = 0; i < numSlots; ++i)
    {
        if(d[i] != kUnknown) continue;
        path.clear();
        uint32_t s = i, base = 0;
        for(;;)
        {
            d[s] = kOnPath;
            path.push_back(s);
            const int32_t t = targets[s];
            if(t < 0) { base = 0; break; }
            if(d[size_t(t)] == kOnPath) return false;       // the chain comes back to itself
            if(d[size_t(t)] != kUnknown) { base = d[size_t(t)] + 1u; break; }
            s = uint32_t(t);
        }
        for(size_t k = path.size(); k-- > 0; ) d[path[k]] = base++;
    }

    uint32_t maxDepth = 0;
    for(uint32_t v : d) if(v > maxDepth) maxDepth = v;
    uint32_t n = 0;
    for(uint32_t level = maxDepth + 1u; level-- > 0; )
        for(uint32_t i = 0; i < numSlots; ++i)
            if(d[i] == level) order[n++] = i;
    if(depth) for(uint32_t i = 0; i < numSlots; ++i) depth[i] = d[i];
    return true;
}

} // namespace oalgpu
