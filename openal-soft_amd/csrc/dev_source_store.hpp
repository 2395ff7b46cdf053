// How the parameter stage's kernels (SourceParamsKernel, ChannelParamsKernel, AmbiParamsKernel) write a ParamRecord, once: the
// record's 283 dwords leave in five passes of 64, lane l storing dword l + 64 * pass -- one coalesced dword store per pass.  A
// head dword (the voice, mStep, the resampler, FilterActive, the send slots) is a uniform value picked by comparisons; a dword
// of the filters comes from the lane that designed the filter (lane k < 14: filter k, SourceFilterDesign) by a cross-lane read;
// a dword of dryGains / sendGains is the pan gain of that line (PanLineGain); the hrtfIdx dwords are getCoeffs' index half
// (HrtfBlendFor).  Nothing is indexed at run time, so nothing leaves the registers.  StoreParamRecord is the whole record of a
// voice that is panned by a direction (a ChannelPan: the two pan-gain kernels); AmbiParamsKernel forms its line gains from a
// matrix row and takes the pieces.
#pragma once
#include <stddef.h>
#include "dev_source_channels.hpp"

#pragma clang fp contract(off)

namespace oalgpu {

constexpr uint32_t kRecordDwords = sizeof(ParamRecord) / 4u;
constexpr uint32_t kRecordPasses = (kRecordDwords + 63u) / 64u;
constexpr uint32_t kOffFilters = offsetof(ParamRecord, dirLp) / 4u;         // dirLp | dirHp | sendLp[6] | sendHp[6]: 14 x 5
constexpr uint32_t kOffHrtfDir = offsetof(ParamRecord, hrtfDir) / 4u;
constexpr uint32_t kOffDryGains = offsetof(ParamRecord, dryGains) / 4u;
constexpr uint32_t kOffSendGains = offsetof(ParamRecord, sendGains) / 4u;
constexpr uint32_t kOffHrtfIdx = offsetof(ParamRecord, hrtfIdx) / 4u;
static_assert(kRecordDwords == 283 && kOffFilters == 14 && kOffHrtfDir == kOffFilters + 70 && kOffDryGains == kOffHrtfDir + 5
    && kOffSendGains == kOffDryGains + 32 && kOffHrtfIdx == kOffSendGains + 150 && kOffHrtfIdx + 12 == kRecordDwords,
    "the parameter stage stores ParamRecord dword by dword");

__device__ __forceinline__ uint32_t Bits(float f) { return __builtin_bit_cast(uint32_t, f); }

// dword d < kOffFilters
__device__ __forceinline__ uint32_t RecordHeadDword(uint32_t d, uint32_t voice, const SourceGains &g, const ResamplerPrep &rs, uint32_t flags)
{
    switch(d)
    {
    case 0: return voice;
    case 1: return g.step;
    case 2: return uint32_t(rs.kind);
    case 3: return rs.m;
    case 4: return rs.l;
    case 5: return Bits(rs.sf);
    case 6: return rs.filterOffset;
    case 7: return flags;
    default: return uint32_t(Pick6(g.sendSlot, d - 8u));
    }
}

// dword kOffFilters <= d < kOffHrtfDir from the lane that designed its filter (c: this lane's design).  Every lane of the
// wavefront calls this, before any branch on d: all of them take part in the cross-lane reads; for another d the value is unused.
__device__ __forceinline__ uint32_t RecordFilterDword(uint32_t d, const float (&c)[5])
{
    const uint32_t f = (d >= kOffFilters && d < kOffHrtfDir) ? d - kOffFilters : 0u;
    const int owner = int(f / 5u);
    const uint32_t j = f % 5u;
    const float c0 = __shfl(c[0], owner), c1 = __shfl(c[1], owner), c2 = __shfl(c[2], owner), c3 = __shfl(c[3], owner),
        c4 = __shfl(c[4], owner);
    return Bits(j == 0u ? c0 : (j == 1u ? c1 : (j == 2u ? c2 : (j == 3u ? c3 : c4))));
}

// dword kOffHrtfIdx + k
__device__ __forceinline__ uint32_t RecordHrtfIdxDword(uint32_t k, const HrirBlend &b)
{
    switch(k)
    {
    case 0: return b.idx[0];
    case 1: return b.idx[1];
    case 2: return b.idx[2];
    case 3: return b.idx[3];
    case 4: return Bits(b.w[0]);
    case 5: return Bits(b.w[1]);
    case 6: return Bits(b.w[2]);
    case 7: return Bits(b.w[3]);
    case 8: return Bits(b.passthru);
    case 9: return b.delay[0];
    case 10: return b.delay[1];
    default: return 0u;                     // keepHrtf: the stage always computes the target
    }
}

// the record of one voice panned to pan.dir, by the whole wavefront (c: this lane's filter design, zeros in lanes >= 14)
__device__ __forceinline__ void StoreParamRecord(uint32_t *dst, uint32_t lane, uint32_t voice, const SourceGains &g,
    const ResamplerPrep &rs, uint32_t flags, const float (&c)[5], const ChannelPan &pan, const HrirBlend &b, const SourceSetup &cx)
{
    // CalcDirectionCoeffs: OpenAL -> ambisonic coordinates (core/mixer.h:71-72)
    const float ay = -pan.dir[0], az = pan.dir[1], ax = -pan.dir[2];
    const float dryGain = g.dryBase * pan.pangain;
#pragma unroll
    for(uint32_t pass = 0; pass < kRecordPasses; ++pass)
    {
        const uint32_t d = lane + 64u * pass;
        uint32_t v = 0u;
        const uint32_t filter = RecordFilterDword(d, c);
        if(d < kOffFilters) v = RecordHeadDword(d, voice, g, rs, flags);
        else if(d < kOffHrtfDir) v = filter;
        else if(d < kOffDryGains)
        {
            const uint32_t k = d - kOffHrtfDir;
            v = Bits(k == 0u ? pan.hrtfEv : (k == 1u ? pan.hrtfAz : (k == 2u ? pan.hrtfDist : (k == 3u ? pan.hrtfSpread : dryGain))));
        }
        else if(d < kOffSendGains)
        {   // ComputePanGains(&Device->Dry, coeffs, DryGain.Base * pangain, ...): dry-line contexts (an HRTF voice has no dry gains)
            const uint32_t t = d - kOffDryGains;
            float gain = 0.0f;
            if(!cx.hrtf && !pan.silent && t < cx.numDry)
                gain = PanLineGain(cx.dryMap[t].index, cx.dryMap[t].scale, ay, az, ax, pan.drySpread, dryGain);
            v = Bits(gain);
        }
        else if(d < kOffHrtfIdx)
        {   // ComputePanGains(&Slot->Wet, coeffs, WetGain[s].Base * pangain, ...) of the sends that have a slot
            const uint32_t k = d - kOffSendGains, s = k / 25u, wc = k % 25u;
            const int32_t sendSlot = Pick6(g.sendSlot, s);
            float gain = 0.0f;
            if(sendSlot >= 0 && !pan.silent && wc < cx.wetChannels)
            {
                const AmbiMapEntry m = cx.wetMaps[size_t(sendSlot) * cx.wetChannels + wc];
                gain = PanLineGain(m.index, m.scale, ay, az, ax, pan.sendSpread, Pick6(g.wetBase, s) * pan.pangain);
            }
            v = Bits(gain);
        }
        else v = RecordHrtfIdxDword(d - kOffHrtfIdx, b);
        if(d < kRecordDwords) dst[d] = v;
    }
}

} // namespace oalgpu
