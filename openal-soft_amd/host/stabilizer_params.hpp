// Host-side constants of the front stabilizer (CreateStablizer, alc/panning.cpp:160-172; the pan constants of
// DeviceBase::Process(StablizerPostProcess), alc/alu.cpp:384-387) and InitDistanceComp's arithmetic
// (alc/panning.cpp:301-371).  See stabilizer_params.cpp.
#pragma once
#include <stdint.h>

namespace oalgpu {

constexpr uint32_t kDistCompMaxDelay = 1023u;      // DistanceComp::MaxDelay - 1

// What the stabilizer kernel reads: BandSplitter::init's coefficient (the mid filter's and every channel filter's) and the
// four pan constants, raised here with the host libm -- the reference's own bits.
struct StabilizerConsts {
    float coeff{0.0f};
    float midLf{0.0f}, midHf{0.0f}, centerLf{0.0f}, centerHf{0.0f};
};

// false unless 0 < xover_norm < 0.5
bool StabilizerDerive(float xoverNorm, StabilizerConsts *out);

// InitDistanceComp for n channels in float, as the reference computes it: delays[i] = floor((maxdist - d) * (rate / 343.3f)
// + 0.5f) clamped to kDistCompMaxDelay and gains[i] = d / maxdist; 0 and 1 for a channel with d <= 0.  True if any delay is
// non-zero (the reference's total > 0); with maxdist <= 0 every channel gets 0 and 1.
bool DistanceCompDerive(uint32_t sampleRate, const float *distances, uint32_t n, uint32_t *delays, float *gains);

} // namespace oalgpu
