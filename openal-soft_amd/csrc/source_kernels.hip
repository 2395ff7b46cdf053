// The parameter stage of moved sources on the GPU: SourceParamsKernel turns source records (292 bytes: the voice, its
// frequency, the VoiceProps subset of oalgpu_source_props) into ParamRecords in device memory, complete in every field, for
// ApplyParamsKernel, BlendRowsKernel, the voice kernels' in-kernel installs and the resident doorbell to consume unchanged.
// The arithmetic is dev_source.hpp's (CalcAttnVoiceParams + CalcPanningAndFilters for a mono 3D point source), the same
// functions oalgpu_source_params_host compiles for the host.
//
// One wavefront per record.  The scalar chain (transform, distance model, cone, clamps, absorption, decay, Doppler, step,
// resampler, spread, HRTF direction and getCoeffs' index half) is uniform across the wavefront and every lane computes it:
// nothing is broadcast.  The fan-out is by lane: lane k < 14 designs filter k (a divergent region of 14 lanes: one sin, one
// cos, two sqrt, five divisions each); then the record's 283 dwords leave in five passes of 64, lane l storing dword
// l + 64 * pass -- one coalesced dword store per pass -- where a dword of the filters comes from the designing lane by a
// cross-lane read, a dword of dryGains / sendGains is the pan gain of that line (PanLineGain), and the rest are the uniform
// values.  No LDS, no scratch (tests/test_source_kernel_resources.py).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stddef.h>
#include "dev_source.hpp"

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
    "SourceParamsKernel stores ParamRecord dword by dword");

__device__ __forceinline__ uint32_t Bits(float f) { return __builtin_bit_cast(uint32_t, f); }

__global__ void __launch_bounds__(64) SourceParamsKernel(SourceSetup cx, HrtfStoreDev st, oalgpu_listener_params lis,
    const SourceRecord *__restrict__ recs, ParamRecord *__restrict__ out)
{
    const SourceRecord &rec = recs[blockIdx.x];
    const oalgpu_source_props &p = rec.p;
    const uint32_t lane = threadIdx.x;

    const SourceGains g = SourceAttenuation(p, rec.frequency, lis, cx);
    const ResamplerPrep rs = PrepareResamplerDev(*cx.rs, p.resampler, g.step);
    const uint32_t flags = SourceFilterFlags(g, cx.numSends);
    HrirBlend b{};
    if(cx.hrtf) b = HrtfBlendFor(st, g.hrtfEv, g.hrtfAz, g.hrtfDist, g.spread);

    float c[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if(lane < 14u) SourceFilterDesign(lane, p, g, cx, c);

    // CalcDirectionCoeffs: OpenAL -> ambisonic coordinates (core/mixer.h:71-72)
    const float ay = -g.dir[0], az = g.dir[1], ax = -g.dir[2];
    uint32_t *dst = reinterpret_cast<uint32_t*>(out + blockIdx.x);
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
            case 0: v = rec.voice; break;
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
            v = Bits(k == 0u ? g.hrtfEv : (k == 1u ? g.hrtfAz : (k == 2u ? g.hrtfDist : (k == 3u ? g.spread : g.dryBase))));
        }
        else if(d < kOffSendGains)
        {   // ComputePanGains(&Device->Dry, coeffs, DryGain.Base, ...): dry-line contexts (an HRTF voice has no dry gains)
            const uint32_t t = d - kOffDryGains;
            float gain = 0.0f;
            if(!cx.hrtf && t < cx.numDry) gain = PanLineGain(cx.dryMap[t].index, cx.dryMap[t].scale, ay, az, ax, g.spread, g.dryBase);
            v = Bits(gain);
        }
        else if(d < kOffHrtfIdx)
        {   // ComputePanGains(&Slot->Wet, coeffs, WetGain[s].Base, ...) of the sends that have a slot
            const uint32_t k = d - kOffSendGains, s = k / 25u, ch = k % 25u;
            const int32_t slot = Pick6(g.sendSlot, s);
            float gain = 0.0f;
            if(slot >= 0 && ch < cx.wetChannels)
            {
                const AmbiMapEntry m = cx.wetMaps[size_t(slot) * cx.wetChannels + ch];
                gain = PanLineGain(m.index, m.scale, ay, az, ax, g.spread, Pick6(g.wetBase, s));
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

void LaunchSourceParams(hipStream_t s, const SourceSetup &cx, const HrtfStoreDev &st, const oalgpu_listener_params &listener,
    const SourceRecord *recs, uint32_t count, ParamRecord *out, hipEvent_t evStart, hipEvent_t evStop)
{
    if(!count) return;
    if(evStart || evStop)
        hipExtLaunchKernelGGL(SourceParamsKernel, dim3(count), dim3(64), 0, s, evStart, evStop, 0, cx, st, listener, recs, out);
    else
        hipLaunchKernelGGL(SourceParamsKernel, dim3(count), dim3(64), 0, s, cx, st, listener, recs, out);
}

} // namespace oalgpu
