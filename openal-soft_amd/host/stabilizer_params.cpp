// CreateStablizer's filter coefficient and the pan constants of DeviceBase::Process(StablizerPostProcess) restated: the
// reference takes std::cos / std::sin of float arguments, so the host libm's float functions give its bits.
// InitDistanceComp restated operation for operation in float.
#include "stabilizer_params.hpp"

#include <algorithm>
#include <cmath>

#include "params.hpp"

namespace oalgpu {

bool StabilizerDerive(float xoverNorm, StabilizerConsts *out)
{
    if(!(xoverNorm > 0.0f && xoverNorm < 0.5f)) return false;
    const float halfPi = 3.14159265358979323846f * 0.5f;
    StabilizerConsts k{};
    k.coeff = SplitterCoeff(xoverNorm);
    // the low band goes 1/3 of the way to the centre, the high band 1/4 (alu.cpp:384-387)
    k.midLf = std::cos(1.0f / 3.0f * halfPi);
    k.midHf = std::cos(1.0f / 4.0f * halfPi);
    k.centerLf = std::sin(1.0f / 3.0f * halfPi);
    k.centerHf = std::sin(1.0f / 4.0f * halfPi);
    *out = k;
    return true;
}

bool DistanceCompDerive(uint32_t sampleRate, const float *distances, uint32_t n, uint32_t *delays, float *gains)
{
    for(uint32_t i = 0; i < n; ++i) { delays[i] = 0u; gains[i] = 1.0f; }
    if(n == 0) return false;
    const float maxdist = *std::max_element(distances, distances + n);
    if(!(maxdist > 0.0f)) return false;
    const float distSampleScale = float(sampleRate) / 343.3f;      // SpeedOfSoundMetersPerSec
    bool any = false;
    for(uint32_t i = 0; i < n; ++i)
    {
        const float distance = distances[i];
        float delay = std::floor((maxdist - distance) * distSampleScale + 0.5f);
        if(delay > float(kDistCompMaxDelay)) delay = float(kDistCompMaxDelay);
        if(distance > 0.0f)
        {
            delays[i] = uint32_t(delay);
            gains[i] = distance / maxdist;
        }
        any = any || delays[i] != 0u;
    }
    return any;
}

} // namespace oalgpu
