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
// the record leaves through StoreParamRecord (dev_source_store.hpp).  No LDS, no scratch (tests/test_channel_kernel_resources.py).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "dev_source_store.hpp"

#pragma clang fp contract(off)

namespace oalgpu {
namespace {

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

    // (the channel's own inputs are read after the source's chain, the voice and the record's place here: what is read early stays
    // in scalar registers across SourceAttenuation, which leaves none free)
    const uint32_t voice = rec.voices[ch];
    uint32_t *dst = reinterpret_cast<uint32_t*>(out + (rec.outBase + uint32_t(__builtin_popcount(rec.present & ((1u << ch) - 1u)))));
    StoreParamRecord(dst, lane, voice, g, rs, flags, c, pan, b, cx);
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
