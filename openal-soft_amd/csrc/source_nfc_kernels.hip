// The near-field side of the source stage on the GPU: SourceNfcKernel turns the source records the params kernels read
// (SourceRecord: SourceParamsKernel's, ChannelSourceRecord: ChannelParamsKernel's) into one NfcRecord per channel voice -- the
// w0 CalcNormalPanning hands to NfcFilter::adjust and the fourteen coefficients adjust leaves -- and ApplyNfcKernel installs
// such records.  The arithmetic is dev_source_nfc.hpp's on top of dev_source.hpp's, the same functions
// oalgpu_channel_source_nfc_host compiles for the host.
//
// One wavefront per source.  It takes the route's chain only as far as the distance: SourceAttenuation is called, and of its
// results only `distance` is used, so what the compiler keeps of it is the listener transform and normalize()'s root (no pow,
// acos, asin, no slot environment).  w0 is the same in every lane; lanes 0..5 then design the six sections (a division for the
// w0, two per section in the instruction stream), and lanes 0..14 collect the record's dwords from them: the orders' gain
// products and the coefficients, by cross-lane reads.  The source's channel voices all get the same fifteen dwords but for the
// voice index, in the params kernels' output order (outBase + the channels before this one that have a voice).  The voices,
// `present` and `outBase` are read after the chain (what is read early stays in scalar registers across it).  No LDS, no
// scratch (tests/test_nfc_kernel_resources.py).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stddef.h>
#include "dev_source_nfc.hpp"

#pragma clang fp contract(off)

namespace oalgpu {
namespace {

static_assert(offsetof(NfcRecord, a0) == 4 && offsetof(NfcRecord, b) == 20, "SourceNfcKernel stores NfcRecord dword by dword");

__device__ __forceinline__ uint32_t Bits(float f) { return __builtin_bit_cast(uint32_t, f); }

__global__ void __launch_bounds__(64) SourceNfcKernel(SourceSetup cx, oalgpu_listener_params lis, NfcSetup nfc,
    const SourceRecord *__restrict__ mono, const ChannelSourceRecord *__restrict__ chan, NfcRecord *__restrict__ out)
{
    const uint32_t lane = threadIdx.x;
    const bool isMono = mono != nullptr;
    const oalgpu_source_props &p = isMono ? mono[blockIdx.x].p : chan[blockIdx.x].p;
    const uint32_t frequency = isMono ? mono[blockIdx.x].frequency : chan[blockIdx.x].frequency;
    // CalcVoiceParams' route (a SourceRecord is a mono 3D point source: attenuated); CalcNonAttnVoiceParams pans with distance 0
    const bool attenuated = isMono || SourceRoute(chan[blockIdx.x].channels, chan[blockIdx.x].spatialize);
    const float distance = attenuated ? SourceAttenuation(p, frequency, lis, cx).distance : 0.0f;
    const float w0 = SourceNfcW0(distance, lis.nfc_scale, nfc.avgSpeakerDist, cx.sampleRate);

    // the six sections, one per lane (the lanes above them repeat section 0: every lane takes part in the cross-lane reads)
    float c1, c2;
    const float g = NfcSectionDesign(lane < kNfcSections ? lane : 0u, 0.5f * w0, c1, c2);

    // dword d of the record, d = lane: 0 the voice, 1..4 a[o][0] of order o = d, 5..14 the packed b
    const uint32_t d = lane < kNfcRecordDwords ? lane : 0u;
    const uint32_t o = (d >= 1u && d <= 4u) ? d : 1u;
    const uint32_t first = NfcFirstSection(o);
    const float g1 = __shfl(g, int(first)), g0 = __shfl(g, int(first + 1u));
    const float gain = o >= 3u ? g1 * g0 : g1;
    const float base = o == 1u ? nfc.baseGain[0] : (o == 2u ? nfc.baseGain[1] : (o == 3u ? nfc.baseGain[2] : nfc.baseGain[3]));
    const float a0 = base * gain;                           // mBaseGain * g (NfcFilterAdjustN)
    // b's entry k comes from section 0 | 1 1 | 2 2 3 | 4 4 5 (a nibble each), its second coefficient where the bit is set
    const uint32_t k = d >= 5u ? d - 5u : 0u;
    const int section = int((0x5544322110ull >> (4u * k)) & 0xfull);
    const float s1 = __shfl(c1, section), s2 = __shfl(c2, section);
    const float bk = ((0x294u >> k) & 1u) ? s2 : s1;
    const uint32_t word = Bits(d >= 5u ? bk : a0);

    const uint32_t present = isMono ? 1u : chan[blockIdx.x].present;
    const uint32_t outBase = isMono ? blockIdx.x : chan[blockIdx.x].outBase;
    uint32_t *dst = reinterpret_cast<uint32_t*>(out + outBase);
    for(uint32_t ch = 0; ch < OALGPU_MAX_SOURCE_CHANNELS; ++ch)
    {
        if(!((present >> ch) & 1u)) continue;
        const uint32_t voice = isMono ? mono[blockIdx.x].voice : chan[blockIdx.x].voices[ch];
        if(lane < kNfcRecordDwords) dst[lane] = lane == 0u ? voice : word;
        dst += kNfcRecordDwords;
    }
}

// NFCtrlFilter.adjust + VoiceFlag::HasNfc of `count` voices: thread (record, cell) writes one of the fifty cells of NfcState::a
// and ::b as oalgpu_voice_set_nfc leaves them (a[o][0] and b[o][1..o] from the record, a[o][1..o] the device filter's, zero
// elsewhere); NfcState::z, the filter's history, is not touched
__global__ void __launch_bounds__(256) ApplyNfcKernel(DeviceLayout L, NfcDeviceCoeffs deviceA, const NfcRecord *__restrict__ recs, uint32_t count)
{
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, t = threadIdx.x & 63u;
    if(i >= count || t >= 50u) return;
    const NfcRecord &r = recs[i];
    const uint32_t v = r.voice;
    if(v >= L.numVoices) return;
    const bool isB = t >= 25u;
    const uint32_t cell = isB ? t - 25u : t, o = cell / 5u, kk = cell % 5u;
    float x = 0.0f;
    if(o >= 1u && kk >= 1u && kk <= o) x = isB ? r.b[NfcPacked(o, kk)] : deviceA.a[NfcPacked(o, kk)];
    else if(o >= 1u && kk == 0u && !isB) x = r.a0[o - 1u];
    float *dst = isB ? &L.nfc[v].b[0][0] : &L.nfc[v].a[0][0];
    dst[cell] = x;
    if(t == 0u) L.ctl[v].flags |= kFlagNfc;
}

} // namespace

void LaunchSourceNfc(hipStream_t s, const SourceSetup &cx, const oalgpu_listener_params &listener, const NfcSetup &nfc,
    const SourceRecord *mono, const ChannelSourceRecord *chan, uint32_t count, NfcRecord *out, hipEvent_t evStart, hipEvent_t evStop)
{
    if(!count) return;
    if(evStart || evStop)
        hipExtLaunchKernelGGL(SourceNfcKernel, dim3(count), dim3(64), 0, s, evStart, evStop, 0, cx, listener, nfc, mono, chan, out);
    else
        hipLaunchKernelGGL(SourceNfcKernel, dim3(count), dim3(64), 0, s, cx, listener, nfc, mono, chan, out);
}

void LaunchApplyNfc(hipStream_t s, const DeviceLayout &L, const NfcDeviceCoeffs &deviceA, const NfcRecord *recs, uint32_t count)
{
    if(!count || !L.nfc) return;
    hipLaunchKernelGGL(ApplyNfcKernel, dim3((count + 3u) / 4u), dim3(256), 0, s, L, deviceA, recs, count);
}

} // namespace oalgpu
