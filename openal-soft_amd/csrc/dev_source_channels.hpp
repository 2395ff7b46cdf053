// The parameter stage of multi-channel and non-spatialized sources, once, for the device (ChannelParamsKernel,
// source_channel_kernels.hip) and for the host (oalgpu_channel_source_params_host, api_sources.hip): CalcVoiceParams' route
// (alc/alu.cpp:2024-2030, DirectChannels off), CalcNonAttnVoiceParams (:1659-1710), and what the multi-channel legs of
// CalcHrtfPanning (:1229-1310) and CalcNormalPanning (:1365-1465, not Pairwise) do with one channel of the maps (:1471-1521).
// The attenuated route is dev_source.hpp's SourceAttenuation, called, not restated.
//
//   SourceNonAttenuation   mStep without Doppler, srcgain = clamp(Gain, min(MinGain, MaxGain), MaxGain), the dry and the send
//                          gains under the listener gain and the GainMixMax ceiling, HF / LF straight from the filters; the
//                          direction CalcPanningAndFilters(0, 0, -1, distance 0, spread 0) has
//   SourceRoute            which of the two a source takes
//   ChannelPanning         one channel: its map position (StereoPan for stereo: {-sin(a), 0, -cos(a)}, always recomputed) and
//                          pangain (GetPanGainSelector, :1079-1113); with distance > epsilon the position warped towards the
//                          source -- a = 1 - 1/(2 pi) * spread, lerpf(chan.pos, (x, y, z), a), divided by its length below 1 --
//                          and no spread anywhere; without, the map position itself, an infinite HRTF distance, spreadmult = 0
//                          for getCoeffs and the dry-line pans, and `spread` for an HRTF context's sends (:1302, not
//                          spreadmult: kept).  The LFE channel is silent (its one audible case needs Dry.Buffer ==
//                          RealOut.Buffer, which no context of this library has).  A MONO source keeps SourceGains' direction,
//                          its spread everywhere and pangain 1: the record SourceParamsKernel writes.
//
// Filters, FilterActive, mStep and the resampler are the source's: SourceFilterDesign, SourceFilterFlags and
// PrepareResamplerDev of dev_source.hpp on the route's SourceGains, equal in every channel voice (copyParamsFrom,
// :1632-1636).  No contraction, no fmaf, as dev_source.hpp: mStep and FilterActive equal the reference's bit for bit.
#pragma once
#include "dev_source.hpp"

#pragma clang fp contract(off)

namespace oalgpu {

// a channel source as the kernel reads it: SourceRecord's fields for all its channel voices, which channels have a voice (bit
// c: channel c) and where the source's records start in the output (the channels with a voice, in channel order, follow each
// other), and the rest of oalgpu_channel_source
struct ChannelSourceRecord {
    uint32_t frequency, present, outBase;
    int32_t channels, spatialize;
    float stereoPan[2], panning;
    uint32_t voices[OALGPU_MAX_SOURCE_CHANNELS];
    oalgpu_source_props p;
};
static_assert(sizeof(ChannelSourceRecord) == 348, "ChannelSourceRecord");

// what CalcPanningAndFilters pans one channel with
struct ChannelPan {
    bool silent;                    // LFE: an all-zero target
    float dir[3];                   // the argument of CalcDirectionCoeffs (OpenAL space)
    float pangain;
    float hrtfEv, hrtfAz, hrtfDist, hrtfSpread;     // getCoeffs' arguments (HRTF contexts)
    float drySpread, sendSpread;    // CalcDirectionCoeffs' spread for the dry bus and for the sends
};

__host__ __device__ __forceinline__ uint32_t SourceChannelCount(int32_t channels)
{
    return channels == OALGPU_CHANNELS_MONO ? 1u : (channels <= OALGPU_CHANNELS_REAR ? 2u : (channels == OALGPU_CHANNELS_QUAD ? 4u
        : (channels == OALGPU_CHANNELS_X51 ? 6u : (channels == OALGPU_CHANNELS_X61 ? 7u : 8u))));
}

// CalcVoiceParams, alu.cpp:2024-2030 with DirectChannels off: true = CalcAttnVoiceParams
__host__ __device__ __forceinline__ bool SourceRoute(int32_t channels, int32_t spatialize)
{
    return !(spatialize == OALGPU_SPATIALIZE_OFF || (spatialize == OALGPU_SPATIALIZE_AUTO && channels != OALGPU_CHANNELS_MONO));
}

// CalcNonAttnVoiceParams, alu.cpp:1659-1710, up to its call of CalcPanningAndFilters(0, 0, -1, 0, 0, ...)
__host__ __device__ __forceinline__ SourceGains SourceNonAttenuation(const oalgpu_source_props &p, uint32_t frequency,
    const oalgpu_listener_params &lis, const SourceSetup &cx)
{
    constexpr float kGainMixMax = 1000.0f;                  // alc/alu.h:18
    SourceGains g;
#pragma unroll
    for(uint32_t s = 0; s < 6; ++s)
    {
        const int32_t slot = p.send[s].slot;
        g.sendSlot[s] = (s < cx.numSends && slot >= 0 && uint32_t(slot) < cx.numSlots && cx.slotEnv[slot].active) ? slot : -1;
    }

    const float pitch = float(frequency) / float(cx.sampleRate) * p.pitch;
    if(pitch > 10.0f) g.step = 10u << kFracBits;            // MaxPitch, core/voice.h:33
    else
    {
        const uint32_t st = fastf2u(pitch * float(kFracOne));
        g.step = st > 1u ? st : 1u;
    }

    const float mingain = (p.max_gain < p.min_gain) ? p.max_gain : p.min_gain;
    const float srcgain = SrcClamp(p.gain, mingain, p.max_gain);
    {
        const float x = srcgain * p.direct_gain * lis.gain;
        g.dryBase = (x < kGainMixMax) ? x : kGainMixMax;
    }
    g.dryHF = p.direct_gain_hf;
    g.dryLF = p.direct_gain_lf;
#pragma unroll
    for(uint32_t s = 0; s < 6; ++s)
    {
        const float x = srcgain * p.send[s].gain * lis.gain;
        g.wetBase[s] = (x < kGainMixMax) ? x : kGainMixMax;
        g.wetHF[s] = p.send[s].gain_hf;
        g.wetLF[s] = p.send[s].gain_lf;
    }

    g.distance = 0.0f; g.spread = 0.0f;
    g.dir[0] = 0.0f; g.dir[1] = 0.0f; g.dir[2] = -1.0f;
    g.hrtfEv = 0.0f; g.hrtfAz = 0.0f; g.hrtfDist = __builtin_inff();
    return g;
}

// the position (x, z; y is 0 in every map) and the side (0: left, 1: right, 2: centre, 3: LFE) of channel c of a layout,
// alu.cpp:892-897, :1471-1521 -- by comparisons, so that nothing is indexed at run time
__host__ __device__ __forceinline__ void ChannelMapEntry(int32_t channels, uint32_t c, const float (&stereoPan)[2], float &x, float &z,
    uint32_t &side)
{
    constexpr float sin30 = 0.5f, cos30 = 0.866025403785f;
    constexpr float sin45 = 1.41421356237309504880f * 0.5f, cos45 = 1.41421356237309504880f * 0.5f;
    constexpr float sin110 = 0.939692620786f, cos110 = -0.342020143326f;
    const bool right = (c & 1u) != 0u;
    x = 0.0f; z = -1.0f; side = 2u;                         // FrontCenter: MonoMap
    if(channels == OALGPU_CHANNELS_STEREO)
    {
        const float a = right ? stereoPan[1] : stereoPan[0];
        x = -sinf(a); z = -cosf(a); side = right ? 1u : 0u;
    }
    else if(channels == OALGPU_CHANNELS_REAR)
    {
        x = right ? sin30 : -sin30; z = cos30; side = right ? 1u : 0u;
    }
    else if(channels == OALGPU_CHANNELS_QUAD)
    {
        x = right ? sin45 : -sin45; z = (c < 2u) ? -cos45 : cos45; side = right ? 1u : 0u;
    }
    else if(channels >= OALGPU_CHANNELS_X51)
    {
        if(c < 2u) { x = right ? sin30 : -sin30; z = -cos30; side = right ? 1u : 0u; }
        else if(c == 2u) { }
        else if(c == 3u) { x = 0.0f; z = 0.0f; side = 3u; }
        else if(channels == OALGPU_CHANNELS_X51) { x = right ? sin110 : -sin110; z = -cos110; side = right ? 1u : 0u; }
        else if(channels == OALGPU_CHANNELS_X61)
        {
            if(c == 4u) { x = 0.0f; z = 1.0f; }             // BackCenter
            else { x = (c == 6u) ? 1.0f : -1.0f; z = 0.0f; side = (c == 6u) ? 1u : 0u; }
        }
        else if(c < 6u) { x = right ? sin30 : -sin30; z = cos30; side = right ? 1u : 0u; }
        else { x = right ? 1.0f : -1.0f; z = 0.0f; side = right ? 1u : 0u; }
    }
}

// a channel's place, which does not depend on the source's gains: the map entry and the balance
struct ChannelSeat { uint32_t side /* ChannelMapEntry's; 4: a MONO source */; float x, z, pangain; };

__host__ __device__ __forceinline__ ChannelSeat ChannelSeatOf(int32_t channels, uint32_t c, const float (&stereoPan)[2], float panning)
{
    ChannelSeat r;
    uint32_t side;
    ChannelMapEntry(channels, c, stereoPan, r.x, r.z, side);
    if(channels == OALGPU_CHANNELS_MONO) side = 4u;
    r.side = side;
    const float one_minus = 1.0f - panning, one_plus = 1.0f + panning;
    const float lgain = (1.0f < one_minus) ? 1.0f : one_minus;              // std::min(1 - Panning, 1)
    const float rgain = (1.0f < one_plus) ? 1.0f : one_plus;
    const float mingain = (rgain < lgain) ? rgain : lgain;
    r.pangain = side == 4u ? 1.0f : (side == 0u ? lgain : (side == 1u ? rgain : (side == 2u ? mingain : 0.0f)));
    return r;
}

__host__ __device__ __forceinline__ ChannelPan ChannelPanning(const ChannelSeat &seat, const SourceGains &g, uint32_t hrtf)
{
    ChannelPan r;
    r.silent = seat.side == 3u;
    r.pangain = seat.pangain;
    if(seat.side == 4u)
    {   // the mono 3D point source's legs (:1209-1227, :1343-1362) and MonoMap's single position without distance: dev_source.hpp
        r.dir[0] = g.dir[0]; r.dir[1] = g.dir[1]; r.dir[2] = g.dir[2];
        r.hrtfEv = g.hrtfEv; r.hrtfAz = g.hrtfAz; r.hrtfDist = g.hrtfDist; r.hrtfSpread = g.spread;
        r.drySpread = g.spread; r.sendSpread = g.spread;
        return r;
    }
    r.hrtfEv = 0.0f; r.hrtfAz = 0.0f; r.hrtfDist = g.hrtfDist; r.hrtfSpread = 0.0f;
    r.drySpread = 0.0f; r.sendSpread = 0.0f;
    r.dir[0] = seat.x; r.dir[1] = 0.0f; r.dir[2] = seat.z;
    if(r.silent) return r;
    if(g.distance > kFltEpsilon)
    {
        const float a = 1.0f - (0.318309886183790671538f * 0.5f) * g.spread;
        r.dir[0] = SrcLerp(seat.x, g.dir[0], a); r.dir[1] = SrcLerp(0.0f, g.dir[1], a); r.dir[2] = SrcLerp(seat.z, g.dir[2], a);
        const float len = sqrtf(r.dir[0] * r.dir[0] + r.dir[1] * r.dir[1] + r.dir[2] * r.dir[2]);
        if(len < 1.0f)
        {
            r.dir[0] /= len; r.dir[1] /= len; r.dir[2] /= len;
        }
        if(hrtf)
        {
            r.hrtfEv = asinf(SrcClamp(r.dir[1], -1.0f, 1.0f));
            r.hrtfAz = atan2f(r.dir[0], -r.dir[2]);
        }
    }
    else
    {
        r.hrtfDist = __builtin_inff();
        if(hrtf)
        {
            r.hrtfEv = asinf(r.dir[1]);
            r.hrtfAz = atan2f(r.dir[0], -r.dir[2]);
            r.sendSpread = g.spread;                        // CalcDirectionCoeffs(chans[c].pos, spread), alu.cpp:1302
        }
    }
    return r;
}

// ---- launcher (source_channel_kernels.hip): `count` channel sources -> the ParamRecords of their channel voices, one
// wavefront each, at out[rec.outBase ...]; maxChannels: the largest channel count among them (every record's `present` bits lie
// below it); evStart / evStop: events bound to the dispatch (null: none) ----
void LaunchChannelParams(hipStream_t s, const SourceSetup &cx, const HrtfStoreDev &st, const oalgpu_listener_params &listener,
    const ChannelSourceRecord *recs, uint32_t count, uint32_t maxChannels, ParamRecord *out, hipEvent_t evStart = nullptr, hipEvent_t evStop = nullptr);

} // namespace oalgpu
