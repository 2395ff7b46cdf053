// The device's side of ProcessContexts (alc/alu.cpp:2177-2273): the table oalgpu_context_attach / _detach build for a device
// context, and the one launch per post-processing update that walks it (bus_merge_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace oalgpu {

// a contributor of a destination line: one line of an attached context's bus block, and the row of the line's next
// contributor in attach order (-1: the last)
struct BusMergeRow {
    const float *src;
    int32_t next;
    uint32_t pad;
};

// a destination line somebody maps to (one workgroup each): the device context's line and its first contributor's row
struct BusMergeHead {
    float *dst;
    int32_t first;
    uint32_t pad;
};

// frames [0, samplesToDo) of every head's line: own value + contributors in table order, one fp32 add each
void LaunchBusMerge(hipStream_t s, const BusMergeHead *heads, const BusMergeRow *rows, uint32_t numHeads, uint32_t samplesToDo);

} // namespace oalgpu
