// Host-side constants of the bs2b crossfeed (init() of core/bs2b.cpp:41-83): the low-pass and high-boost coefficients of a
// level at a sample rate.  See crossfeed_params.cpp.
#pragma once
#include <stdint.h>

namespace oalgpu {

// What the crossfeed kernel reads, in bs2b_processor's member order
struct CrossfeedConsts {
    float a0Lo{0.0f}, b1Lo{0.0f};
    float a0Hi{0.0f}, a1Hi{0.0f}, b1Hi{0.0f};
};

// false unless 1 <= level <= 6 (Bs2b::LowCLevel .. HighECLevel: what alc/panning.cpp:1424 lets through) and sampleRate >= 1
bool CrossfeedDerive(int level, uint32_t sampleRate, CrossfeedConsts *out);

} // namespace oalgpu
