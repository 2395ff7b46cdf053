// ProcessContexts' sum over the contexts of a device (alc/alu.cpp:2177-2273): every context mixes into the device's one
// MixBuffer.  Here every attached context has a bus block of its own, and BusMergeKernel adds their dry + real lines into the
// device context's behind its reduction: one launch per post-processing update, a workgroup per destination line that
// somebody maps to.  A workgroup walks its line's contributors in attach order (the table oalgpu_context_attach built), so a
// sample's value is ((own + c0) + c1) + ... whatever else runs: no atomics, the same bits every time.
//
// The launch sits on the device context's post stream beside the next update's voice kernel: no LDS, no scratch, a handful of
// registers -- a wavefront finds room on any SIMD the voice wavefronts leave 16 registers of.
#include "bus_merge.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace oalgpu {
namespace {

constexpr uint32_t kMergeThreads = kLine / 4u;      // a lane per four frames of the line: 128-bit loads and stores

// (the table hands out generic pointers; the lines are device memory: global loads and stores, not flat ones)
typedef float f4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) f4 *gfloat4p;
typedef const __attribute__((address_space(1))) f4 *gcfloat4p;
typedef __attribute__((address_space(1))) float *gfloatp;

// A line's contributors are a chain: each row is a scalar load that depends on the row before it, then a vector load.  That
// serialises long chains -- a handful of contexts per device is what this is for.
__global__ __launch_bounds__(kMergeThreads) void BusMergeKernel(const BusMergeHead *__restrict__ heads,
    const BusMergeRow *__restrict__ rows, uint32_t n)
{
    const BusMergeHead head = heads[blockIdx.x];
    const uint32_t i = threadIdx.x * 4u;
    if(i >= n) return;
    // (the lines are 1024 frames long and 4 KB aligned: the last vector of a partial update is read whole)
    const gfloatp dst = reinterpret_cast<gfloatp>(reinterpret_cast<uint64_t>(head.dst)) + i;
    f4 acc = *reinterpret_cast<gcfloat4p>(dst);
    for(int32_t r = head.first; r >= 0;)
    {
        const BusMergeRow row = rows[r];
        const f4 v = *reinterpret_cast<gcfloat4p>(reinterpret_cast<uint64_t>(row.src + i));
        acc.x = acc.x + v.x; acc.y = acc.y + v.y; acc.z = acc.z + v.z; acc.w = acc.w + v.w;
        r = row.next;
    }
    if(i + 4u <= n) *reinterpret_cast<gfloat4p>(dst) = acc;
    else
    {   // only frames below samples_to_do are written
        dst[0] = acc.x;
        if(i + 1u < n) dst[1] = acc.y;
        if(i + 2u < n) dst[2] = acc.z;
    }
}

} // namespace

void LaunchBusMerge(hipStream_t s, const BusMergeHead *heads, const BusMergeRow *rows, uint32_t numHeads, uint32_t samplesToDo)
{
    if(!numHeads) return;
    hipLaunchKernelGGL(BusMergeKernel, dim3(numHeads), dim3(kMergeThreads), 0, s, heads, rows, samplesToDo);
}

} // namespace oalgpu
