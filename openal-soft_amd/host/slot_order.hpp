// The processing order of effect slots that feed other slots (AL_EFFECTSLOT_TARGET_SOFT): what the slot sort of ProcessContexts
// (alc/alu.cpp:2220-2249) establishes, as depths.  See slot_order.cpp.
#pragma once
#include <stdint.h>

namespace oalgpu {

// targets[i]: the slot that slot i's effect output adds into, -1: the device's lines.
// depth[i] (may be null): 0 for a slot without a target, otherwise its target's depth + 1.
// order[0 .. numSlots): the slots by descending depth, within one depth by ascending index -- every slot in front of its target.
// false, with order and depth untouched: a target out of range (below -1 or >= numSlots), a slot that targets itself, a cycle.
bool SlotOrder(const int32_t *targets, uint32_t numSlots, uint32_t *order, uint32_t *depth);

} // namespace oalgpu
