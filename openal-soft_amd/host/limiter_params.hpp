// Host-side derivation of the output limiter's constants: Compressor::Create (core/mastering.cpp) and the device
// limiter UpdateDeviceParams builds (alc/alc.cpp:1079-1090, 1750-1768).  See limiter_params.cpp.
#pragma once
#include <stdint.h>

#include "../../include/oalgpu.h"

namespace oalgpu {

enum : uint32_t {
    kLimAutoKnee = 1u, kLimAutoAttack = 2u, kLimAutoRelease = 4u, kLimAutoPostGain = 8u, kLimAutoDeclip = 16u
};

// What the limiter kernel reads: Compressor's members after Create, with gainCompressor's starting attack / release
// coefficients (exp(-1/attack), exp(-1/(release - attack))) raised here with the host libm -- the reference's own.
struct LimiterConsts {
    uint32_t numChans{0};
    uint32_t lookAhead{0};
    uint32_t hold{0};                  // the sliding hold's length; 0 where Create makes none (look-ahead 0, or hold <= 1)
    uint32_t flags{0};                 // kLimAuto*; Declip only together with PostGain (as mAuto.Declip)
    float preGain{1.0f}, postGain{0.0f}, threshold{0.0f}, slope{0.0f}, knee{0.0f};
    float attack{1.0f}, release{1.0f};
    float crestCoeff{0.0f}, gainEstimate{0.0f}, adaptCoeff{0.0f};
    float attackCoeff{0.0f}, releaseCoeff{0.0f};
};

// false for parameters Create cannot take (a sample rate that is not positive and finite, non-finite times)
bool LimiterDerive(const oalgpu_limiter_params &p, LimiterConsts *out);
// CreateDeviceLimiter with the threshold of alc.cpp:1750-1768; true where the format enables it by default
bool LimiterDeviceParams(uint32_t sampleRate, int sampleType, float ditherDepth, oalgpu_limiter_params *out);

} // namespace oalgpu
