// Parameter design shared by the host and the device: the shelf / peaking / pass filter design of BiquadFilter::SetParams
// (core/filters/biquad.cpp:48-129) behind setParamsFromSlope (biquad.h:172-177), and BsincPrepare's scale index and
// interpolation factor (alc/alu.cpp:140-164).  host/params.cpp compiles this file as plain C++ (glibc's sinf / cosf / sqrtf),
// csrc/source_kernels.hip as device code (the device math library's): the same operations in the same order, no contraction.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/oalgpu.h"

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define OALGPU_HD __host__ __device__
#else
#define OALGPU_HD
#endif

#pragma clang fp contract(off)

namespace oalgpu {

// BiquadFilter::SetParams: b0, b1, b2, a1, a2 (a0-normalised) into c[5]
OALGPU_HD inline void DesignBiquad(int type, float f0norm, float gain, float rcpQ, float c[5])
{
    gain = (gain < 0.00001f) ? 0.00001f : gain;          // SetParams: -100 dB floor
    const float w0 = 3.14159265358979323846f * 2.0f * ((0.49f < f0norm) ? 0.49f : f0norm);
    const float sw = sinf(w0), cw = cosf(w0);
    const float alpha = sw / 2.0f * rcpQ;
    float a0 = 1.0f, a1 = 0.0f, a2 = 0.0f, b0 = 1.0f, b1 = 0.0f, b2 = 0.0f;
    switch(type)
    {
    case OALGPU_BIQUAD_HIGHSHELF:
        {
            const float sa = 2.0f * sqrtf(gain) * alpha;
            b0 = gain * ((gain + 1.0f) + (gain - 1.0f) * cw + sa);
            b1 = -2.0f * gain * ((gain - 1.0f) + (gain + 1.0f) * cw);
            b2 = gain * ((gain + 1.0f) + (gain - 1.0f) * cw - sa);
            a0 = (gain + 1.0f) - (gain - 1.0f) * cw + sa;
            a1 = 2.0f * ((gain - 1.0f) - (gain + 1.0f) * cw);
            a2 = (gain + 1.0f) - (gain - 1.0f) * cw - sa;
        }
        break;
    case OALGPU_BIQUAD_LOWSHELF:
        {
            const float sa = 2.0f * sqrtf(gain) * alpha;
            b0 = gain * ((gain + 1.0f) - (gain - 1.0f) * cw + sa);
            b1 = 2.0f * gain * ((gain - 1.0f) - (gain + 1.0f) * cw);
            b2 = gain * ((gain + 1.0f) - (gain - 1.0f) * cw - sa);
            a0 = (gain + 1.0f) + (gain - 1.0f) * cw + sa;
            a1 = -2.0f * ((gain - 1.0f) + (gain + 1.0f) * cw);
            a2 = (gain + 1.0f) + (gain - 1.0f) * cw - sa;
        }
        break;
    case OALGPU_BIQUAD_PEAKING:
        b0 = 1.0f + alpha * gain; b1 = -2.0f * cw; b2 = 1.0f - alpha * gain;
        a0 = 1.0f + alpha / gain; a1 = -2.0f * cw; a2 = 1.0f - alpha / gain;
        break;
    case OALGPU_BIQUAD_LOWPASS:
        b0 = (1.0f - cw) / 2.0f; b1 = 1.0f - cw; b2 = (1.0f - cw) / 2.0f;
        a0 = 1.0f + alpha; a1 = -2.0f * cw; a2 = 1.0f - alpha;
        break;
    case OALGPU_BIQUAD_HIGHPASS:
        b0 = (1.0f + cw) / 2.0f; b1 = -(1.0f + cw); b2 = (1.0f + cw) / 2.0f;
        a0 = 1.0f + alpha; a1 = -2.0f * cw; a2 = 1.0f - alpha;
        break;
    case OALGPU_BIQUAD_BANDPASS:
        b0 = alpha; b1 = 0.0f; b2 = -alpha;
        a0 = 1.0f + alpha; a1 = -2.0f * cw; a2 = 1.0f - alpha;
        break;
    }
    c[0] = b0 / a0; c[1] = b1 / a0; c[2] = b2 / a0; c[3] = a1 / a0; c[4] = a2 / a0;
}

// setParamsFromSlope: rcpQFromSlope (biquad.h:60-62) in front of SetParams
OALGPU_HD inline void DesignBiquadFromSlope(int type, float f0norm, float gain, float slope, float c[5])
{
    gain = (gain < 0.001f) ? 0.001f : gain;              // setParamsFromSlope: -60 dB floor
    DesignBiquad(type, f0norm, gain, sqrtf((gain + 1.0f / gain) * (1.0f / slope - 1.0f) + 2.0f), c);
}

// BsincPrepare for increment > MixerFracOne: the scale index into the table's m[] / filterOffset[] and the curve-fitted
// interpolation factor between that scale and the next
OALGPU_HD inline void BsincScale(float scaleBase, float scaleRange, uint32_t increment, uint32_t &si, float &sf)
{
    sf = float(1u << OALGPU_MIXER_FRAC_BITS) / float(increment) - scaleBase;
    sf = 16.0f * sf * scaleRange - 1.0f;
    sf = (0.0f < sf) ? sf : 0.0f;
    si = uint32_t(sf);                                   // float2uint of a value in [0, 15]: truncation
    sf -= float(si);
    sf = 1.0f - sqrtf(1.0f - sf * sf);
}

} // namespace oalgpu
