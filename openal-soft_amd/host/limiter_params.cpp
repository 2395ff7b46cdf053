// Compressor::Create (core/mastering.cpp) and CreateDeviceLimiter / its threshold (alc/alc.cpp:1079-1090,
// 1750-1768) restated, operation for operation in the reference's precisions: float where it computes in
// float (round, pow, exp), double where it converts dB to nepers.
#include "limiter_params.hpp"

#include <algorithm>
#include <cmath>

namespace oalgpu {

bool LimiterDerive(const oalgpu_limiter_params &p, LimiterConsts *out)
{
    if(!(p.sample_rate > 0.0f) || !std::isfinite(p.sample_rate) || !std::isfinite(p.look_ahead_time)
        || !std::isfinite(p.hold_time))
        return false;
    LimiterConsts k{};
    const float kMax = float(1024 - 1);
    const uint32_t lookAhead = uint32_t(std::clamp(std::round(p.look_ahead_time * p.sample_rate), 0.0f, kMax));
    const uint32_t hold = uint32_t(std::clamp(std::round(p.hold_time * p.sample_rate), 0.0f, kMax));
    const uint32_t f = p.auto_flags;
    k.flags = f & (kLimAutoKnee | kLimAutoAttack | kLimAutoRelease | kLimAutoPostGain);
    if((f & kLimAutoPostGain) && (f & kLimAutoDeclip)) k.flags |= kLimAutoDeclip;
    k.numChans = p.num_channels;
    k.lookAhead = lookAhead;
    k.preGain = std::pow(10.0f, p.pre_gain_db / 20.0f);
    k.postGain = float(std::log(10.0) / 20.0 * double(p.post_gain_db));
    k.threshold = float(std::log(10.0) / 20.0 * double(p.threshold_db));
    k.slope = 1.0f / std::max(1.0f, p.ratio) - 1.0f;
    k.knee = float(std::max(0.0, std::log(10.0) / 20.0 * double(p.knee_db)));
    k.attack = std::max(1.0f, p.attack_time * p.sample_rate);
    k.release = std::max(1.0f, p.release_time * p.sample_rate);
    if(f & kLimAutoKnee) k.slope = -1.0f;
    // (the sliding hold does not take a length of 1; without a look-ahead there is neither hold nor delay)
    k.hold = (lookAhead > 0 && hold > 1) ? hold : 0u;
    k.crestCoeff = std::exp(-1.0f / (0.200f * p.sample_rate));
    k.gainEstimate = k.threshold * -0.5f * k.slope;
    k.adaptCoeff = std::exp(-1.0f / (2.0f * p.sample_rate));
    // gainCompressor's t_att / t_rel before any automation (what it keeps without AutoAttack / AutoRelease)
    const float t_att = k.attack;
    const float t_rel = k.release - k.attack;
    k.attackCoeff = std::exp(-1.0f / t_att);
    k.releaseCoeff = std::exp(-1.0f / t_rel);
    *out = k;
    return true;
}

bool LimiterDeviceParams(uint32_t sampleRate, int sampleType, float ditherDepth, oalgpu_limiter_params *out)
{
    // DevFmtType order: Byte, UByte, Short, UShort, Int, UInt, Float
    float thrshld = 1.0f;
    if(sampleType == OALGPU_OUT_I8 || sampleType == OALGPU_OUT_U8) thrshld = 127.0f / 128.0f;
    else if(sampleType == OALGPU_OUT_I16 || sampleType == OALGPU_OUT_U16) thrshld = 32767.0f / 32768.0f;
    if(ditherDepth > 0.0f) thrshld -= 1.0f / ditherDepth;
    const float thrshld_dB = std::log10(thrshld) * 20.0f;
    oalgpu_limiter_params p{};
    p.num_channels = 0;
    p.sample_rate = float(sampleRate);
    p.auto_flags = kLimAutoKnee | kLimAutoAttack | kLimAutoRelease | kLimAutoPostGain | kLimAutoDeclip;
    p.look_ahead_time = 0.001f; p.hold_time = 0.002f;
    p.pre_gain_db = 0.0f; p.post_gain_db = 0.0f;
    p.threshold_db = thrshld_dB;
    p.ratio = INFINITY;
    p.knee_db = 0.0f;
    p.attack_time = 0.02f; p.release_time = 0.2f;
    *out = p;
    return sampleType != OALGPU_OUT_F32;
}

} // namespace oalgpu
