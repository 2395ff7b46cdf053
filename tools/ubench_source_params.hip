// SourceParamsKernel alone: `count` source records -> `count` ParamRecords, timed by events bound to the dispatch (median of 50
// launches after 5 warm-ups), for an HRTF context with one send (BASELINE configs[2]'s layout) or a dry-line context with
// two.  With a layout (oalgpu_source_channels, 1 = stereo .. 6 = 7.1): ChannelParamsKernel over `count` sources of that layout
// (spatialize on: the attenuated chain) and, beside it in the same run, SourceParamsKernel at the same number of records.  The kernel and its launcher are the library's own translation unit; the HRTF store is a synthetic one of the golden
// set's shape (19 elevations x 24 azimuths, one field): the kernel reads its index arrays and delays, never the responses.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-math-errno -fgpu-flush-denormals-to-zero \
//       -o tools/ubench_source_params tools/ubench_source_params.hip openal-soft_amd/csrc/source_kernels.hip \
//       openal-soft_amd/csrc/source_channel_kernels.hip openal-soft_amd/host/tables.cpp
//   tools/ubench_source_params [count = 1024] [hrtf = 1] [layout = -1: SourceParamsKernel only]
// One JSON line per kernel.  Beside the keys the line has always had (kernel, records, hrtf, median_us, min_us, max_us, bytes_in,
// bytes_out, step0) it names `sources` and `layout` (-1: source records) and the voice of the last record, `last_voice`: that
// the ragged output order ended where it should.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../openal-soft_amd/csrc/dev_source_channels.hpp"
#include "../openal-soft_amd/host/tables.hpp"

using namespace oalgpu;

#define CHECK(x) do { hipError_t e_ = (x); if(e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while(0)

template<typename T>
static T *Upload(const std::vector<T> &v)
{
    T *p = nullptr;
    if(hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(v.size(), 1) * sizeof(T)) != hipSuccess) return nullptr;
    if(!v.empty() && hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return p;
}

int main(int argc, char **argv)
{
    const uint32_t count = argc > 1 ? uint32_t(std::atoi(argv[1])) : 1024u;
    const bool hrtf = argc > 2 ? std::atoi(argv[2]) != 0 : true;
    const int layout = argc > 3 ? std::atoi(argv[3]) : -1;
    if(count == 0 || count > (1u << 20) || layout > OALGPU_CHANNELS_X71) { std::fprintf(stderr, "count or layout out of range\n"); return 1; }
    const uint32_t channels = layout >= 0 ? SourceChannelCount(layout) : 1u;
    const uint32_t records = count * channels;
    if(records > (1u << 20)) { std::fprintf(stderr, "more than 2^20 records\n"); return 1; }
    uint32_t seed = 0x5EED0054u;
    auto uniform = [&seed](float lo, float hi) { seed = seed * 1664525u + 1013904223u; return lo + (hi - lo) * float(seed / 4294967296.0); };

    ResamplerConsts rs{};
    uint32_t at = 0;
    const int fam[3] = {12, 24, 48};
    for(int f = 0; f < 3; ++f)
    {
        const BsincTable *t = GetBsincTable(fam[f]);
        rs.fam[f].scaleBase = t->scaleBase; rs.fam[f].scaleRange = t->scaleRange;
        std::memcpy(rs.fam[f].m, t->m, sizeof(t->m));
        std::memcpy(rs.fam[f].filterOffset, t->filterOffset, sizeof(t->filterOffset));
        rs.bsincBase[f] = at; at += uint32_t(t->tab.size());
    }
    rs.cubicBase[0] = at; rs.cubicBase[1] = at + 256u;

    const uint32_t numSends = hrtf ? 1u : 2u, numSlots = numSends, numDry = hrtf ? 4u : 5u, wet = 4u;
    std::vector<oalgpu_slot_environment> env(numSlots, oalgpu_slot_environment{1, 0.0f, 1.49f, 0.994f});
    std::vector<AmbiMapEntry> dryMap(numDry), wetMaps(numSlots * wet);
    for(uint32_t i = 0; i < numDry; ++i) dryMap[i] = AmbiMapEntry{i, 1.0f};
    for(uint32_t i = 0; i < numSlots * wet; ++i) wetMaps[i] = AmbiMapEntry{i % wet, 1.0f};
    // the store: one field, 19 elevations of 24 azimuths
    const uint32_t evCount = 19, azCount = 24;
    std::vector<float> fieldDistance{1.0f};
    std::vector<uint8_t> fieldEvCount{uint8_t(evCount)}, delays(evCount * azCount * 2);
    std::vector<uint16_t> elevAzCount(evCount, uint16_t(azCount)), elevIrOffset(evCount);
    for(uint32_t e = 0; e < evCount; ++e) elevIrOffset[e] = uint16_t(e * azCount);
    for(uint8_t &d : delays) d = uint8_t(uniform(0.0f, 40.0f));

    std::vector<SourceRecord> recs(records);
    for(uint32_t i = 0; i < records; ++i)
    {
        SourceRecord &r = recs[i];
        std::memset(&r, 0, sizeof(r));
        r.voice = i; r.frequency = 44100u;
        oalgpu_source_props &p = r.p;
        p.pitch = uniform(0.6f, 1.6f); p.gain = uniform(0.05f, 1.0f); p.max_gain = 1.0f; p.inner_angle = p.outer_angle = 360.0f;
        p.ref_distance = 1.0f; p.max_distance = 3.4e38f; p.rolloff_factor = 1.0f;
        for(int k = 0; k < 3; ++k) { p.position[k] = uniform(-4.0f, 4.0f); p.velocity[k] = uniform(-5.0f, 5.0f); }
        p.distance_model = OALGPU_DISTANCE_INVERSE_CLAMPED; p.resampler = OALGPU_RESAMPLER_BSINC24;
        p.dry_gain_hf_auto = p.wet_gain_auto = p.wet_gain_hf_auto = 1; p.outer_gain_hf = 1.0f; p.doppler_factor = 1.0f;
        p.air_absorption_factor = (i & 1u) ? 1.0f : 0.0f;
        p.direct_gain = 1.0f; p.direct_gain_hf = (i % 4u == 1u) ? 0.5f : 1.0f; p.direct_hf_reference = 5000.0f; p.direct_gain_lf = 1.0f;
        p.direct_lf_reference = 250.0f;
        for(int s = 0; s < OALGPU_MAX_SENDS; ++s) p.send[s] = oalgpu_source_send{s < int(numSends) ? 0 : -1, 0.5f, 1.0f, 5000.0f, 1.0f, 250.0f};
    }
    oalgpu_listener_params lis{};
    lis.matrix[0] = lis.matrix[5] = lis.matrix[10] = lis.matrix[15] = 1.0f;
    lis.gain = lis.meters_per_unit = lis.doppler_factor = lis.cone_scale = lis.nfc_scale = 1.0f;
    lis.air_absorption_gain_hf = 0.99426f; lis.speed_of_sound = 343.3f; lis.source_distance_model = 1;
    lis.xyz_scale[0] = lis.xyz_scale[1] = lis.xyz_scale[2] = 1.0f;

    HrtfStoreDev st{};
    st.irSize = 32; st.numFields = 1; st.numElevs = evCount; st.numIrs = evCount * azCount;
    st.fieldDistance = Upload(fieldDistance); st.fieldEvCount = Upload(fieldEvCount);
    st.elevAzCount = Upload(elevAzCount); st.elevIrOffset = Upload(elevIrOffset); st.delays = Upload(delays);
    SourceSetup cx{48000u, numSends, numSlots, numDry, wet, hrtf ? 1u : 0u, Upload(env), Upload(std::vector<ResamplerConsts>{rs}),
        Upload(dryMap), Upload(wetMaps)};
    // the channel sources: source i has the props of record i, its channel voices are i * channels ...
    std::vector<ChannelSourceRecord> chans(layout >= 0 ? count : 0u);
    for(uint32_t i = 0; i < uint32_t(chans.size()); ++i)
    {
        ChannelSourceRecord &r = chans[i];
        std::memset(&r, 0, sizeof(r));
        r.frequency = 44100u; r.present = (1u << channels) - 1u; r.outBase = i * channels;
        r.channels = layout; r.spatialize = OALGPU_SPATIALIZE_ON;
        r.stereoPan[0] = 0.5235988f; r.stereoPan[1] = -0.5235988f; r.panning = uniform(-0.5f, 0.5f);
        for(uint32_t c = 0; c < OALGPU_MAX_SOURCE_CHANNELS; ++c) r.voices[c] = c < channels ? i * channels + c : OALGPU_NO_VOICE;
        r.p = recs[i].p;
    }
    SourceRecord *drecs = Upload(recs);
    ChannelSourceRecord *dchans = Upload(chans);
    ParamRecord *out = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void**>(&out), size_t{records} * sizeof(ParamRecord)));
    if(!st.delays || !cx.slotEnv || !cx.rs || !cx.dryMap || !cx.wetMaps || !drecs || !dchans) { std::fprintf(stderr, "allocation failed\n"); return 1; }
    hipStream_t s;
    hipEvent_t e0, e1;
    CHECK(hipStreamCreate(&s)); CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    for(int which = 0; which < (layout >= 0 ? 2 : 1); ++which)
    {
        const bool chan = layout >= 0 && which == 0;
        std::vector<float> us;
        for(int k = 0; k < 55; ++k)
        {
            if(chan) LaunchChannelParams(s, cx, st, lis, dchans, count, channels, out, e0, e1);
            else LaunchSourceParams(s, cx, st, lis, drecs, records, out, e0, e1);
            CHECK(hipGetLastError());
            CHECK(hipStreamSynchronize(s));
            float ms = 0.0f;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            if(k >= 5) us.push_back(ms * 1000.0f);
        }
        std::vector<ParamRecord> back(records);
        CHECK(hipMemcpy(back.data(), out, size_t{records} * sizeof(ParamRecord), hipMemcpyDeviceToHost));
        std::sort(us.begin(), us.end());
        std::printf("{\"kernel\": \"%s\", \"sources\": %u, \"layout\": %d, \"records\": %u, \"hrtf\": %d, \"median_us\": %.2f, "
            "\"min_us\": %.2f, \"max_us\": %.2f, \"bytes_in\": %zu, \"bytes_out\": %zu, \"step0\": %u, \"last_voice\": %u}\n",
            chan ? "ChannelParamsKernel" : "SourceParamsKernel", chan ? count : records, chan ? layout : -1, records, hrtf ? 1 : 0,
            us[us.size() / 2], us.front(), us.back(), chan ? size_t{count} * sizeof(ChannelSourceRecord) : size_t{records} * sizeof(SourceRecord),
            size_t{records} * sizeof(ParamRecord), back[0].step, back[records - 1].voice);
    }
    return 0;
}
