// The parameter stage of B-Format sources on the GPU: AmbiParamsKernel turns ambisonic source records (568 bytes: SourceRecord's
// fields, the spatialize mode, the orientation, the channels' ACN and scale as the host resolved them from layout and scaling,
// the upsampler's place, the channel voices) into one complete ParamRecord per channel voice, for everything that consumes
// ParamRecords to consume unchanged.  The arithmetic is dev_source_ambi.hpp's on top of dev_source_channels.hpp's and
// dev_source.hpp's, the same functions oalgpu_ambi_source_params_host compiles for the host.
//
// One 64-lane workgroup per source.  The route's chain (attenuation or not, step, resampler, filter flags) runs once and is
// the same in every lane; lanes < 14 design the shelves once.  The rotation and the mix matrix sit in LDS (2 x 25 x 25 floats,
// and the 25 panned coefficients): the first-order block is written by lanes < 9, then the bands 2 .. device order run in
// order, a band's (2l + 1)^2 elements spread over the lanes (band 4 has 81: two rounds), a barrier between the bands since
// band l reads band l - 1.  The upsample is one output column per lane (lanes < 25), rows and k in the reference's order; without an
// upsampler the mix matrix is the rotation, copied.  Then, for each channel that has a voice, in channel order: the lanes that hold a dry
// line's or a send line's dword of the record form that gain from the channel's row of the mix matrix, and the record leaves in
// dev_source_store.hpp's passes, its head and filter dwords by that header's pieces; everything but the voice and the gains is
// formed once, before the channels.  Output is dense: record outBase + (the channels before this one that have a voice).
// A source without coverage skips the matrices.  No scratch, no spill (tests/test_ambi_kernel_resources.py).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "dev_source_ambi.hpp"
#include "dev_source_store.hpp"

#pragma clang fp contract(off)

namespace oalgpu {
namespace {

// a[k] for a run-time k without indexing the array
__device__ __forceinline__ float Pick9(const float (&a)[9], uint32_t k)
{
    const float a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5], a6 = a[6], a7 = a[7], a8 = a[8];
    return k == 1u ? a1 : (k == 2u ? a2 : (k == 3u ? a3 : (k == 4u ? a4 : (k == 5u ? a5 : (k == 6u ? a6 : (k == 7u ? a7 : (k == 8u ? a8 : a0)))))));
}

__global__ void __launch_bounds__(64) AmbiParamsKernel(SourceSetup cx, AmbiSetup ambi, oalgpu_listener_params lis,
    const AmbiSourceRecord *__restrict__ recs, ParamRecord *__restrict__ out)
{
    __shared__ float rot[kAmbiMatrix], mix[kAmbiMatrix], panned[kAmbiMax];
    const AmbiSourceRecord &rec = recs[blockIdx.x];
    const oalgpu_source_props &p = rec.p;
    const uint32_t lane = threadIdx.x;

    const bool attenuated = AmbiSourceRoute(rec.spatialize);
    const SourceGains g = attenuated ? SourceAttenuation(p, rec.frequency, lis, cx) : SourceNonAttenuation(p, rec.frequency, lis, cx);
    const ResamplerPrep rs = PrepareResamplerDev(*cx.rs, p.resampler, g.step);
    const uint32_t flags = SourceFilterFlags(g, cx.numSends);
    float c[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if(lane < 14u) SourceFilterDesign(lane, p, g, cx, c);

    const float coverage = AmbiCoverage(g.distance, g.spread);
    const bool covered = coverage > 0.0f;
    {   // CalcDirectionCoeffs(pos, 0): OpenAL -> ambisonic coordinates (core/mixer.h:71-72)
        float pos[3];
        AmbiPanPosition(g, attenuated, pos);
        if(lane < kAmbiMax) panned[lane] = AmbiCoeff(lane, -pos[0], pos[1], -pos[2]);
    }

    // what every channel voice's record shares: all dwords but the voice and the line gains; and of the lanes that hold a line
    // gain's dword: the line's coefficient index, its AmbiMap scale and the gain it is formed under
    uint32_t shared[kRecordPasses], lineIdx[kRecordPasses];
    float lineScale[kRecordPasses], lineGain[kRecordPasses];
#pragma unroll
    for(uint32_t pass = 0; pass < kRecordPasses; ++pass)
    {
        const uint32_t d = lane + 64u * pass;
        uint32_t v = 0u, idx = kAmbiMax;                    // idx == kAmbiMax: not a line of this context
        float scale = 0.0f, gain = 0.0f;
        const uint32_t filter = RecordFilterDword(d, c);
        if(d < kOffFilters) v = RecordHeadDword(d, 0u, g, rs, flags);        // (the voice: per channel, below)
        else if(d < kOffHrtfDir) v = filter;
        else if(d < kOffDryGains) v = 0u;                   // (HRTF contexts are refused: no direction, no Hrtf.Target.Gain)
        else if(d < kOffSendGains)
        {   // ComputePanGains(&Device->Dry, coeffs, DryGain.Base, ...)
            const uint32_t t = d - kOffDryGains;
            if(t < cx.numDry)
            {
                const AmbiMapEntry m = cx.dryMap[t];
                idx = m.index < kAmbiMax ? m.index : kAmbiMax - 1u; scale = m.scale; gain = g.dryBase;
            }
        }
        else if(d < kOffHrtfIdx)
        {   // ComputePanGains(&Slot->Wet, coeffs, WetGain[s].Base, ...) of the sends that have a slot
            const uint32_t k = d - kOffSendGains, s = k / 25u, wc = k % 25u;
            const int32_t sendSlot = Pick6(g.sendSlot, s);
            if(sendSlot >= 0 && wc < cx.wetChannels)
            {
                const AmbiMapEntry m = cx.wetMaps[size_t(sendSlot) * cx.wetChannels + wc];
                idx = m.index < kAmbiMax ? m.index : kAmbiMax - 1u; scale = m.scale; gain = Pick6(g.wetBase, s);
            }
        }
        shared[pass] = v; lineIdx[pass] = idx; lineScale[pass] = scale; lineGain[pass] = gain;
    }

    const uint32_t devChannels = AmbiChannelsOfOrder(ambi.order);
    if(covered)
    {
        for(uint32_t i = lane; i < kAmbiMatrix; i += 64u) rot[i] = 0.0f;
        float block[9];
        const float at[3] = {rec.orientAt[0], rec.orientAt[1], rec.orientAt[2]}, up[3] = {rec.orientUp[0], rec.orientUp[1], rec.orientUp[2]};
        AmbiOrientation(at, up, p.head_relative, lis, block);
        __syncthreads();
        if(lane == 0u) rot[0] = 1.0f;
        if(lane < 9u) rot[(1u + lane / 3u) * kAmbiMax + 1u + lane % 3u] = Pick9(block, lane);
        __syncthreads();
        for(uint32_t l = 2; l <= ambi.order; ++l)
        {
            const uint32_t side = 2u * l + 1u, base = l * l;
            const float *uvw = ambi.rotCoeffs + 3u * AmbiRotatorBandStart(l);
            for(uint32_t e = lane; e < side * side; e += 64u)
            {
                const uint32_t y = e / side, x = e % side;
                rot[(base + y) * kAmbiMax + base + x] = AmbiRotatorElement(rot, uvw + 3u * e, int(l), int(y) - int(l), int(x) - int(l));
            }
            __syncthreads();
        }
        if(rec.upRows)
        {
            if(lane < kAmbiMax)
                for(uint32_t i = 0; i < rec.upRows; ++i)
                    mix[i * kAmbiMax + lane] = AmbiUpsampleEntry(rot, ambi.upsamplers + rec.upOffset + i * kAmbiMax, lane, devChannels);
        }
        else
            for(uint32_t i = lane; i < kAmbiMatrix; i += 64u) mix[i] = rot[i];
    }
    // (the workgroup is one wavefront and `covered` is the same in every lane, so the barriers inside the branch above are met by
    // all lanes or by none; this one publishes `panned` and, with coverage, `mix`)
    __syncthreads();

    // (the channels' inputs are read after the source's chain: what is read early stays in scalar registers across it)
    const float pannedScale = (1.0f - coverage) * rec.scale0;
    const uint32_t present = rec.present;
    uint32_t *dst = reinterpret_cast<uint32_t*>(out + rec.outBase);
    for(uint32_t ch = 0; ch < rec.channels; ++ch)
    {
        if(!((present >> ch) & 1u)) continue;
        const uint32_t voice = rec.voices[ch];
        const uint32_t row = uint32_t(rec.acn[ch]) * kAmbiMax;
        const float scale = rec.scale[ch] * coverage;
#pragma unroll
        for(uint32_t pass = 0; pass < kRecordPasses; ++pass)
        {
            const uint32_t d = lane + 64u * pass;
            uint32_t v = shared[pass];
            if(d == 0u) v = voice;
            const uint32_t idx = lineIdx[pass];
            if(idx < kAmbiMax)
            {
                float gain = 0.0f;
                // (with an upsampler only the rows < upRows = (source order + 1)^2 of `mix` were written; acn is below that for
                // every channel of the format, which the host resolved: no unwritten row is read)
                if(covered)
                    gain = AmbiLineGain(lineScale[pass], AmbiChannelCoeff(mix[row + idx], scale, ch == 0u ? panned[idx] * pannedScale : 0.0f),
                        lineGain[pass]);
                else if(ch == 0u)
                    gain = AmbiLineGain(lineScale[pass], panned[idx], lineGain[pass] * rec.scale0);
                v = Bits(gain);
            }
            if(d < kRecordDwords) dst[d] = v;
        }
        dst += kRecordDwords;
    }
}

} // namespace

void LaunchAmbiParams(hipStream_t s, const SourceSetup &cx, const AmbiSetup &ambi, const oalgpu_listener_params &listener,
    const AmbiSourceRecord *recs, uint32_t count, ParamRecord *out, hipEvent_t evStart, hipEvent_t evStop)
{
    if(!count) return;
    if(evStart || evStop)
        hipExtLaunchKernelGGL(AmbiParamsKernel, dim3(count), dim3(64), 0, s, evStart, evStop, 0, cx, ambi, listener, recs, out);
    else
        hipLaunchKernelGGL(AmbiParamsKernel, dim3(count), dim3(64), 0, s, cx, ambi, listener, recs, out);
}

} // namespace oalgpu
