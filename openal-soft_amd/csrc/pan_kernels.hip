// The panning half of the parameter stage on the GPU: CalcDirectionCoeffs / CalcAmbiCoeffs
// (core/mixer.h:68-73, core/ambidefs.h:219-271, core/mixer.cpp:16-90) and ComputePanGains (core/mixer.cpp:92-102)
// as CalcPanningAndFilters calls them for a point source (alc/alu.cpp: the dry bus with DryGain.Base, every
// send's slot with WetGain[i].Base) -- so that a moving voice's parameter record is a direction, a spread
// and a few gains instead of up to 32 + 6 x 25 resolved line gains.
//
// The encoder coefficients are the real spherical harmonics up to order 4 in ACN order with N3D normalisation;
// thread = one bus line, which evaluates the ONE coefficient its AmbiMap entry names, in the reference's
// operation order (no contraction), so that a direction without spread yields bit-identical gains.  The
// spread's zonal scaling uses cos and sqrt: within an ulp or two of the host's libm.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "dev_pan.hpp"              // AmbiCoeff, SpreadFactor, PanLineGain: shared with SourceParamsKernel and the host

#pragma clang fp contract(off)

namespace oalgpu {
namespace {

// one workgroup per record; thread t < numDry: dry line t; then numSends x wetChannels send lines
__global__ void __launch_bounds__(256) PanGainsKernel(DeviceLayout L, const PanRecord *recs, const AmbiMapEntry *dryMap,
    const AmbiMapEntry *wetMaps /* [slot][wetChannels] */)
{
    const PanRecord r = recs[blockIdx.x];
    const uint32_t v = r.voice, t = threadIdx.x;
    // CalcDirectionCoeffs: OpenAL -> ambisonic coordinates (core/mixer.h:71-72)
    const float y = -r.dir[0], z = r.dir[1], x = -r.dir[2];
    auto gainFor = [&](const AmbiMapEntry &m, float ingain) { return PanLineGain(m.index, m.scale, y, z, x, r.spread, ingain); };
    if(!L.hrtf && t < L.numDry) L.gainTgt[size_t{v} * L.numDry + t] = gainFor(dryMap[t], r.dryGain);
    const uint32_t nsend = L.numSends * L.wetChannels;
    if(t >= 64u && t - 64u < nsend)
    {
        const uint32_t k = t - 64u, s = k / L.wetChannels, c = k % L.wetChannels;
        const int32_t slot = L.ctl[v].sendSlot[s];
        // (a send without a slot keeps mSend[i].Buffer empty: its gains are never read)
        L.sendTgt[size_t{v} * nsend + k] = slot >= 0 ? gainFor(wetMaps[size_t(slot) * L.wetChannels + c], r.sendGain[s]) : 0.0f;
    }
}

} // namespace

void LaunchPanGains(hipStream_t s, const DeviceLayout &L, const PanRecord *recs, uint32_t count, const AmbiMapEntry *dryMap,
    const AmbiMapEntry *wetMaps)
{ hipLaunchKernelGGL(PanGainsKernel, dim3(count), dim3(256), 0, s, L, recs, dryMap, wetMaps); }

} // namespace oalgpu
