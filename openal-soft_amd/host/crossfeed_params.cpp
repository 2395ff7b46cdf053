// init() of core/bs2b.cpp restated operation for operation in float: the reference evaluates the whole expression in single
// precision and takes std::exp of a float argument, so the host libm's expf gives its bits.
#include "crossfeed_params.hpp"

#include <cmath>

namespace oalgpu {

bool CrossfeedDerive(int level, uint32_t sampleRate, CrossfeedConsts *out)
{
    // Fc_lo, Fc_hi, G_lo, G_hi per level (bs2b.cpp:45-66)
    static const float table[6][4] = {
        {360.0f,  501.0f, 0.398107170553497f, 0.205671765275719f},      // low
        {500.0f,  711.0f, 0.459726988530872f, 0.228208484414988f},      // middle
        {700.0f, 1021.0f, 0.530884444230988f, 0.250105790667544f},      // high
        {360.0f,  494.0f, 0.316227766016838f, 0.168236228897329f},      // low, easy
        {500.0f,  689.0f, 0.354813389233575f, 0.187169483835901f},      // middle, easy
        {700.0f,  975.0f, 0.398107170553497f, 0.205671765275719f},      // high, easy
    };
    if(level < 1 || level > 6 || sampleRate < 1u || sampleRate > 0x7fffffffu) return false;
    const float fcLo = table[level - 1][0], fcHi = table[level - 1][1];
    const float gLo = table[level - 1][2], gHi = table[level - 1][3];
    const float srate = float(int(sampleRate));
    const float pi = 3.14159265358979323846f;
    const float g = 1.0f / (1.0f - gHi + gLo);
    CrossfeedConsts k{};
    float x = std::exp(-pi * 2.0f * fcLo / srate);
    k.b1Lo = x;
    k.a0Lo = gLo * (1.0f - x) * g;
    x = std::exp(-pi * 2.0f * fcHi / srate);
    k.b1Hi = x;
    k.a0Hi = (1.0f - gHi * (1.0f - x)) * g;
    k.a1Hi = -x * g;
    *out = k;
    return true;
}

} // namespace oalgpu
