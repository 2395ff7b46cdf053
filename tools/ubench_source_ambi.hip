// AmbiParamsKernel alone: `count` ambisonic sources of `order` (3D, ACN / SN3D, spatialize on: the attenuated chain, a radius so
// that the matrices are built) on a fourth-order dry-line context with one send -> their (order + 1)^2 ParamRecords each, timed
// by events bound to the dispatch (median of 50 launches after 5 warm-ups).  The kernel and its launcher are the library's own
// translation unit; the upsampler is a synthetic one (the kernel's time does not depend on its values).
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-math-errno -fgpu-flush-denormals-to-zero \
//       -fno-slp-vectorize -mllvm -disable-vector-combine -o tools/ubench_source_ambi tools/ubench_source_ambi.hip \
//       openal-soft_amd/csrc/source_ambi_kernels.hip openal-soft_amd/host/tables.cpp
//   tools/ubench_source_ambi [count = 64] [order = 3]
// One JSON line: kernel, sources, order, records, median_us, min_us, max_us, bytes_in, bytes_out, step0, last_voice (that the
// dense output ended where it should).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../openal-soft_amd/csrc/dev_source_ambi.hpp"
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
    const uint32_t count = argc > 1 ? uint32_t(std::atoi(argv[1])) : 64u;
    const uint32_t order = argc > 2 ? uint32_t(std::atoi(argv[2])) : 3u;
    if(count == 0 || count > 4096u || order < 1u || order > 3u) { std::fprintf(stderr, "count (1..4096) or order (1..3) out of range\n"); return 1; }
    const uint32_t channels = AmbiChannelsOfOrder(order), records = count * channels, deviceOrder = 4u;
    uint32_t seed = 0x5EED0075u;
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

    const uint32_t numSends = 1u, numSlots = 1u, numDry = kAmbiMax, wet = 4u;
    std::vector<oalgpu_slot_environment> env(numSlots, oalgpu_slot_environment{1, 0.0f, 1.49f, 0.994f});
    std::vector<AmbiMapEntry> dryMap(numDry), wetMaps(numSlots * wet);
    for(uint32_t i = 0; i < numDry; ++i) dryMap[i] = AmbiMapEntry{i, 1.0f};
    for(uint32_t i = 0; i < numSlots * wet; ++i) wetMaps[i] = AmbiMapEntry{i % wet, 1.0f};
    // RotatorCoeffs as the library computes them (the zeros decide which terms an element has, and keep its reads inside the bands)
    std::vector<float> rotCoeffs(size_t{kRotatorCoeffs} * 3u), upsampler(kAmbiMatrix);
    FillAmbiRotatorCoeffs(rotCoeffs.data());
    for(float &v : upsampler) v = uniform(-0.5f, 0.5f);

    std::vector<AmbiSourceRecord> recs(count);
    for(uint32_t i = 0; i < count; ++i)
    {
        AmbiSourceRecord &r = recs[i];
        std::memset(&r, 0, sizeof(r));
        r.frequency = 44100u; r.present = (1u << channels) - 1u; r.outBase = i * channels;
        r.spatialize = OALGPU_SPATIALIZE_ON; r.channels = channels; r.upRows = channels; r.upOffset = 0u; r.scale0 = 1.0f;
        r.orientAt[0] = uniform(-1.0f, 1.0f); r.orientAt[1] = uniform(-0.2f, 0.2f); r.orientAt[2] = -1.0f;
        r.orientUp[0] = 0.0f; r.orientUp[1] = 1.0f; r.orientUp[2] = 0.0f;
        for(uint32_t c = 0; c < kAmbiMax; ++c)
        {
            r.acn[c] = uint8_t(c < channels ? c : 0u);
            r.scale[c] = 1.7320508f;
            r.voices[c] = c < channels ? i * channels + c : OALGPU_NO_VOICE;
        }
        oalgpu_source_props &p = r.p;
        p.pitch = uniform(0.6f, 1.6f); p.gain = uniform(0.05f, 1.0f); p.max_gain = 1.0f; p.inner_angle = p.outer_angle = 360.0f;
        p.ref_distance = 1.0f; p.max_distance = 3.4e38f; p.rolloff_factor = 1.0f;
        for(int k = 0; k < 3; ++k) { p.position[k] = uniform(-4.0f, 4.0f); p.velocity[k] = uniform(-5.0f, 5.0f); }
        p.radius = 1.5f;
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

    SourceSetup cx{48000u, numSends, numSlots, numDry, wet, 0u, Upload(env), Upload(std::vector<ResamplerConsts>{rs}), Upload(dryMap),
        Upload(wetMaps)};
    AmbiSetup ambi{deviceOrder, Upload(rotCoeffs), Upload(upsampler)};
    AmbiSourceRecord *drecs = Upload(recs);
    ParamRecord *out = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void**>(&out), size_t{records} * sizeof(ParamRecord)));
    if(!cx.slotEnv || !cx.rs || !cx.dryMap || !cx.wetMaps || !ambi.rotCoeffs || !ambi.upsamplers || !drecs) { std::fprintf(stderr, "allocation failed\n"); return 1; }
    hipStream_t s;
    hipEvent_t e0, e1;
    CHECK(hipStreamCreate(&s)); CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    std::vector<float> us;
    for(int k = 0; k < 55; ++k)
    {
        LaunchAmbiParams(s, cx, ambi, lis, drecs, count, out, e0, e1);
        CHECK(hipGetLastError());
        CHECK(hipStreamSynchronize(s));
        float ms = 0.0f;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if(k >= 5) us.push_back(ms * 1000.0f);
    }
    std::vector<ParamRecord> back(records);
    CHECK(hipMemcpy(back.data(), out, size_t{records} * sizeof(ParamRecord), hipMemcpyDeviceToHost));
    std::sort(us.begin(), us.end());
    std::printf("{\"kernel\": \"AmbiParamsKernel\", \"sources\": %u, \"order\": %u, \"records\": %u, \"median_us\": %.2f, \"min_us\": %.2f, "
        "\"max_us\": %.2f, \"bytes_in\": %zu, \"bytes_out\": %zu, \"step0\": %u, \"last_voice\": %u}\n", count, order, records,
        us[us.size() / 2], us.front(), us.back(), size_t{count} * sizeof(AmbiSourceRecord), size_t{records} * sizeof(ParamRecord),
        back[0].step, back[records - 1].voice);
    return 0;
}
