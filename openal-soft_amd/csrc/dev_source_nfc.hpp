// The near-field side of the source stage, once, for the device (SourceNfcKernel, source_nfc_kernels.hip) and for the host
// (oalgpu_channel_source_nfc_host, api_sources.hip): the three AvgSpeakerDist > 0 branches of CalcNormalPanning
// (alc/alu.cpp:1325-1341, :1413-1428) and NfcFilter::adjust (core/filters/nfc.cpp:150-203).
//
//   the distance     what CalcPanningAndFilters receives: SourceGains::distance on the attenuated route (SourceAttenuation,
//                    dev_source.hpp, called, not restated: the listener transform and normalize()), 0 on CalcNonAttnVoiceParams'
//   SourceNfcW0      distance > epsilon: 343.3 / (max(distance * NfcScale, AvgSpeakerDist / 4) * rate); otherwise the "identity"
//                    filter 343.3 / (AvgSpeakerDist * rate) (:1423)
//   adjust(w0)       dev_nfc_design.hpp's six sections; a[o][0] = mBaseGain[o] * (the order's gain factors), b[o][1..o]
//
// Every channel voice of the source gets the same adjust (voice->mChans | take(chans.size()): the LFE channel's too), and
// VoiceFlag::HasNfc.  Only + * / sqrt max and comparisons lie between the source's properties and the coefficients, written
// without contraction and without fmaf as dev_source.hpp's "Exactness" has it: device and host agree bit for bit.
#pragma once
#include "dev_source_channels.hpp"
#include "dev_nfc_design.hpp"

#pragma clang fp contract(off)

namespace oalgpu {

// what the stage reads of a near-field context: DeviceBase::AvgSpeakerDist (oalgpu_context_set_nfc_distance) and mBaseGain of
// the orders 1..4 of DeviceBase::mNFCtrlFilter (oalgpu_context_set_nfc: NfcInit)
struct NfcSetup { float avgSpeakerDist, baseGain[4]; };

// one channel voice's adjust: a[o][0] of the orders 1..4, then b[1][1], b[2][1..2], b[3][1..3], b[4][1..4]
struct NfcRecord { uint32_t voice; float a0[4], b[10]; };
static_assert(sizeof(NfcRecord) == 60, "NfcRecord");
constexpr uint32_t kNfcRecordDwords = sizeof(NfcRecord) / 4u;

// where coefficient k (1..o) of order o (1..4) lies in NfcRecord::b
__host__ __device__ __forceinline__ uint32_t NfcPacked(uint32_t o, uint32_t k) { return o * (o - 1u) / 2u + (k - 1u); }

// the w0 CalcNormalPanning hands to adjust (alu.cpp:1333-1334, :1423)
__host__ __device__ __forceinline__ float SourceNfcW0(float distance, float nfcScale, float avgSpeakerDist, uint32_t sampleRate)
{
    constexpr float kSpeedOfSoundMetersPerSec = 343.3f;     // core/context.h:32
    const float samplerate = float(sampleRate);
    float dist = avgSpeakerDist;
    if(distance > kFltEpsilon)
    {
        const float scaled = distance * nfcScale, least = avgSpeakerDist / 4.0f;
        dist = (scaled < least) ? least : scaled;           // std::max(distance*NfcScale, AvgSpeakerDist/4.0f)
    }
    return kSpeedOfSoundMetersPerSec / (dist * samplerate);
}

// ---- launchers (source_nfc_kernels.hip) ----
// `count` sources -> the NfcRecords of their channel voices, one wavefront per source, in the params kernels' output order:
// record i of `mono` (SourceParamsKernel's input) at out[i], or -- mono null -- the channel voices of chan[i] at
// out[chan[i].outBase ...] (ChannelParamsKernel's input).  evStart / evStop: events bound to the dispatch (null: none)
void LaunchSourceNfc(hipStream_t s, const SourceSetup &cx, const oalgpu_listener_params &listener, const NfcSetup &nfc,
    const SourceRecord *mono, const ChannelSourceRecord *chan, uint32_t count, NfcRecord *out, hipEvent_t evStart = nullptr,
    hipEvent_t evStop = nullptr);
// installs `count` records: L.nfc[voice].a / .b (the a[o][1..o] of the device's filter from deviceA, packed as NfcRecord::b),
// kFlagNfc; the delay elements stay
struct NfcDeviceCoeffs { float a[10]; };
void LaunchApplyNfc(hipStream_t s, const DeviceLayout &L, const NfcDeviceCoeffs &deviceA, const NfcRecord *recs, uint32_t count);

} // namespace oalgpu
