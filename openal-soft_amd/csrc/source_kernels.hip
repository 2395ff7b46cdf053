// The parameter stage of moved sources on the GPU: SourceParamsKernel turns source records (292 bytes: the voice, its
// frequency, the VoiceProps subset of oalgpu_source_props) into ParamRecords in device memory, complete in every field, for
// ApplyParamsKernel, BlendRowsKernel, the voice kernels' in-kernel installs and the resident doorbell to consume unchanged.
// The arithmetic is dev_source.hpp's (CalcAttnVoiceParams + CalcPanningAndFilters for a mono 3D point source), the same
// functions oalgpu_source_params_host compiles for the host.
//
// One wavefront per record.  The scalar chain (transform, distance model, cone, clamps, absorption, decay, Doppler, step,
// resampler, spread, HRTF direction and getCoeffs' index half) is uniform across the wavefront and every lane computes it:
// nothing is broadcast.  The fan-out is by lane: lane k < 14 designs filter k (a divergent region of 14 lanes: one sin, one
// cos, two sqrt, five divisions each); then the record leaves through StoreParamRecord (dev_source_store.hpp), panned as the one
// seat of a MONO channel source: the rule that a mono source is a channel source is dev_source_channels.hpp's ChannelPanning, here
// and in oalgpu_source_params_host.  No LDS, no scratch (tests/test_source_kernel_resources.py).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "dev_source_store.hpp"

#pragma clang fp contract(off)

namespace oalgpu {
namespace {

__global__ void __launch_bounds__(64) SourceParamsKernel(SourceSetup cx, HrtfStoreDev st, oalgpu_listener_params lis,
    const SourceRecord *__restrict__ recs, ParamRecord *__restrict__ out)
{
    const SourceRecord &rec = recs[blockIdx.x];
    const oalgpu_source_props &p = rec.p;
    const uint32_t lane = threadIdx.x;

    const SourceGains g = SourceAttenuation(p, rec.frequency, lis, cx);
    const ResamplerPrep rs = PrepareResamplerDev(*cx.rs, p.resampler, g.step);
    const uint32_t flags = SourceFilterFlags(g, cx.numSends);
    // a mono source is a channel source with MonoMap's one seat (oalgpu_source_params_host says the same): pangain 1, not
    // silent, SourceGains' direction and its spread everywhere
    const float frontPan[2] = {0.0f, 0.0f};
    const ChannelPan pan = ChannelPanning(ChannelSeatOf(OALGPU_CHANNELS_MONO, 0u, frontPan, 0.0f), g, cx.hrtf);
    HrirBlend b{};
    if(cx.hrtf) b = HrtfBlendFor(st, pan.hrtfEv, pan.hrtfAz, pan.hrtfDist, pan.hrtfSpread);

    float c[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if(lane < 14u) SourceFilterDesign(lane, p, g, cx, c);

    StoreParamRecord(reinterpret_cast<uint32_t*>(out + blockIdx.x), lane, rec.voice, g, rs, flags, c, pan, b, cx);
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
