// The parameter stage of multi-channel and non-spatialized sources on the GPU: ChannelParamsKernel turns channel source
// records (348 bytes: SourceRecord's fields, the layout, the spatialize mode, StereoPan, Panning, the channel voices) into
// one complete ParamRecord per channel voice, for everything that consumes ParamRecords to consume unchanged.  The
// arithmetic is dev_source_channels.hpp's on top of dev_source.hpp's, the same functions
// oalgpu_channel_source_params_host compiles for the host.
//
// The grid is count x stride wavefronts, wavefront (source, channel), where stride is the largest channel count among the
// call's sources rounded up to a power of two (a call of stereo sources launches two wavefronts per source, not eight: an
// empty workgroup costs its dispatch: measured 2.8 ns each, 17 us for 1024 stereo sources).  A wavefront whose channel has no voice (the
// layout does not have it, or it is OALGPU_NO_VOICE: the record's `present` bits) leaves at once; the others write record
// outBase + (the source's channels before this one that have a voice), so a call's records are dense whatever the layouts.  The channels of a
// source run beside each other: each repeats the source's uniform chain (route, attenuation or not, step, resampler,
// filter flags) and appends its own short tail (map entry, warp: a lerp, a root, three divisions; asin / atan2 and
// getCoeffs' index half on HRTF contexts).  From there on it is SourceParamsKernel's shape: lanes < 14 design the filters,
// the record's 283 dwords leave in five coalesced passes.  No LDS, no scratch (tests/test_channel_kernel_resources.py).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stddef.h>
#include "dev_source_channels.hpp"

#pragma clang fp contract(off)

namespace oalgpu {
namespace {

constexpr uint32_t kRecordDwords = sizeof(ParamRecord) / 4u;
constexpr uint32_t kOffFilters = offsetof(ParamRecord, dirLp) / 4u;         // dirLp | dirHp | sendLp[6] | sendHp[6]: 14 x 5
constexpr uint32_t kOffHrtfDir = offsetof(ParamRecord, hrtfDir) / 4u;
constexpr uint32_t kOffDryGains = offsetof(ParamRecord, dryGains) / 4u;
constexpr uint32_t kOffSendGains = offsetof(ParamRecord, sendGains) / 4u;
constexpr uint32_t kOffHrtfIdx = offsetof(ParamRecord, hrtfIdx) / 4u;
static_assert(kRecordDwords == 283 && kOffFilters == 14 && kOffHrtfDir == kOffFilters + 70 && kOffDryGains == kOffHrtfDir + 5
    && kOffSendGains == kOffDryGains + 32 && kOffHrtfIdx == kOffSendGains + 150 && kOffHrtfIdx + 12 == kRecordDwords,
    "ChannelParamsKernel stores ParamRecord dword by dword");

__device__ __forceinline__ uint32_t Bits(float f) { return __builtin_bit_cast(uint32_t, f); }

__global__ void __launch_bounds__(64) ChannelParamsKernel(SourceSetup cx, HrtfStoreDev st, oalgpu_listener_params lis,
    const ChannelSourceRecord *__restrict__ recs, ParamRecord *__restrict__ out, uint32_t strideShift)
{
    const ChannelSourceRecord &rec = recs[blockIdx.x >> strideShift];
    const uint32_t ch = blockIdx.x & ((1u << strideShift) - 1u);
    const oalgpu_source_props &p = rec.p;
    const uint32_t lane = threadIdx.x;
    if(!((rec.present >> ch) & 1u)) return;

    const SourceGains g = SourceRoute(rec.channels, rec.spatialize) ? SourceAttenuation(p, rec.frequency, lis, cx)
        : SourceNonAttenuation(p, rec.frequency, lis, cx);
    const ResamplerPrep rs = PrepareResamplerDev(*cx.rs, p.resampler, g.step);
    const uint32_t flags = SourceFilterFlags(g, cx.numSends);
    const float stereoPan[2] = {rec.stereoPan[0], rec.stereoPan[1]};
    const ChannelPan pan = ChannelPanning(ChannelSeatOf(rec.channels, ch, stereoPan, rec.panning), g, cx.hrtf);
    HrirBlend b{};
    if(cx.hrtf && !pan.silent) b = HrtfBlendFor(st, pan.hrtfEv, pan.hrtfAz, pan.hrtfDist, pan.hrtfSpread);

    float c[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if(lane < 14u) SourceFilterDesign(lane, p, g, cx, c);

    // CalcDirectionCoeffs: OpenAL -> ambisonic coordinates (core/mixer.h:71-72)
    const float ay = -pan.dir[0], az = pan.dir[1], ax = -pan.dir[2];
    const float dryGain = g.dryBase * pan.pangain;
    // (the channel's own inputs are read after the source's chain, the voice and the record's place here: what is read early stays
    // in scalar registers across SourceAttenuation, which leaves none free)
    const uint32_t voice = rec.voices[ch];
    uint32_t *dst = reinterpret_cast<uint32_t*>(out + (rec.outBase + uint32_t(__builtin_popcount(rec.present & ((1u << ch) - 1u)))));
#pragma unroll
    for(uint32_t pass = 0; pass < (kRecordDwords + 63u) / 64u; ++pass)
    {
        const uint32_t d = lane + 64u * pass;
        uint32_t v = 0u;
        // the filters' dwords, from the lanes that designed them (every lane takes part in the cross-lane reads)
        const uint32_t f = (d >= kOffFilters && d < kOffHrtfDir) ? d - kOffFilters : 0u;
        const int owner = int(f / 5u);
        const uint32_t j = f % 5u;
        const float c0 = __shfl(c[0], owner), c1 = __shfl(c[1], owner), c2 = __shfl(c[2], owner), c3 = __shfl(c[3], owner),
            c4 = __shfl(c[4], owner);
        if(d < kOffFilters)
        {
            switch(d)
            {
            case 0: v = voice; break;
            case 1: v = g.step; break;
            case 2: v = uint32_t(rs.kind); break;
            case 3: v = rs.m; break;
            case 4: v = rs.l; break;
            case 5: v = Bits(rs.sf); break;
            case 6: v = rs.filterOffset; break;
            case 7: v = flags; break;
            default: v = uint32_t(Pick6(g.sendSlot, d - 8u)); break;
            }
        }
        else if(d < kOffHrtfDir)
            v = Bits(j == 0u ? c0 : (j == 1u ? c1 : (j == 2u ? c2 : (j == 3u ? c3 : c4))));
        else if(d < kOffDryGains)
        {
            const uint32_t k = d - kOffHrtfDir;
            v = Bits(k == 0u ? pan.hrtfEv : (k == 1u ? pan.hrtfAz : (k == 2u ? pan.hrtfDist : (k == 3u ? pan.hrtfSpread : dryGain))));
        }
        else if(d < kOffSendGains)
        {   // ComputePanGains(&Device->Dry, coeffs, DryGain.Base * pangain, ...): dry-line contexts
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
        else
        {
            const uint32_t k = d - kOffHrtfIdx;
            switch(k)
            {
            case 0: v = b.idx[0]; break;
            case 1: v = b.idx[1]; break;
            case 2: v = b.idx[2]; break;
            case 3: v = b.idx[3]; break;
            case 4: v = Bits(b.w[0]); break;
            case 5: v = Bits(b.w[1]); break;
            case 6: v = Bits(b.w[2]); break;
            case 7: v = Bits(b.w[3]); break;
            case 8: v = Bits(b.passthru); break;
            case 9: v = b.delay[0]; break;
            case 10: v = b.delay[1]; break;
            default: v = 0u; break;                // keepHrtf: the stage always computes the target
            }
        }
        if(d < kRecordDwords) dst[d] = v;
    }
}

} // namespace

void LaunchChannelParams(hipStream_t s, const SourceSetup &cx, const HrtfStoreDev &st, const oalgpu_listener_params &listener,
    const ChannelSourceRecord *recs, uint32_t count, uint32_t maxChannels, ParamRecord *out, hipEvent_t evStart, hipEvent_t evStop)
{
    if(!count) return;
    uint32_t strideShift = 0;
    while((1u << strideShift) < maxChannels && strideShift < 3u) ++strideShift;
    const dim3 grid(count << strideShift);
    if(evStart || evStop)
        hipExtLaunchKernelGGL(ChannelParamsKernel, grid, dim3(64), 0, s, evStart, evStop, 0, cx, st, listener, recs, out, strideShift);
    else
        hipLaunchKernelGGL(ChannelParamsKernel, grid, dim3(64), 0, s, cx, st, listener, recs, out, strideShift);
}

} // namespace oalgpu
