// SourceNfcKernel alone, beside SourceParamsKernel in the same run: `count` mono source records of a dry-line context (five dry
// lines, no sends: the near-field device) -> `count` NfcRecords resp. ParamRecords, timed by events bound to the dispatch (median
// of 50 launches after 5 warm-ups), at 1, 64 and 1024 sources.  The kernels and their launchers are the library's own
// translation units.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-math-errno -fgpu-flush-denormals-to-zero \
//       -fno-slp-vectorize -mllvm -disable-vector-combine -o tools/ubench_source_nfc tools/ubench_source_nfc.hip \
//       openal-soft_amd/csrc/source_nfc_kernels.hip openal-soft_amd/csrc/source_kernels.hip openal-soft_amd/host/tables.cpp \
//       openal-soft_amd/host/params.cpp
//   tools/ubench_source_nfc
// One JSON line per kernel and count; `w0_0` and `a0_last` are record 0's w0 as the host computes it and the last record's
// a[4][0] as the kernel left it (that the run computed something).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../openal-soft_amd/csrc/dev_source_nfc.hpp"
#include "../openal-soft_amd/host/params.hpp"
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

int main()
{
    constexpr uint32_t kMax = 1024;
    uint32_t seed = 0x5EED0078u;
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

    const uint32_t numDry = 5u, wet = 4u;
    const uint32_t acn2d[5] = {0u, 1u, 3u, 4u, 8u};
    std::vector<AmbiMapEntry> dryMap(numDry), wetMaps;
    for(uint32_t i = 0; i < numDry; ++i) dryMap[i] = AmbiMapEntry{acn2d[i], 1.0f};
    std::vector<oalgpu_slot_environment> env;

    std::vector<SourceRecord> recs(kMax);
    for(uint32_t i = 0; i < kMax; ++i)
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
        p.direct_gain = 1.0f; p.direct_gain_hf = (i % 4u == 1u) ? 0.5f : 1.0f; p.direct_hf_reference = 5000.0f; p.direct_gain_lf = 1.0f;
        p.direct_lf_reference = 250.0f;
        for(int s = 0; s < OALGPU_MAX_SENDS; ++s) p.send[s] = oalgpu_source_send{-1, 1.0f, 1.0f, 5000.0f, 1.0f, 250.0f};
    }
    oalgpu_listener_params lis{};
    lis.matrix[0] = lis.matrix[5] = lis.matrix[10] = lis.matrix[15] = 1.0f;
    lis.gain = lis.meters_per_unit = lis.doppler_factor = lis.cone_scale = lis.nfc_scale = 1.0f;
    lis.air_absorption_gain_hf = 0.99426f; lis.speed_of_sound = 343.3f; lis.source_distance_model = 1;
    lis.xyz_scale[0] = lis.xyz_scale[1] = lis.xyz_scale[2] = 1.0f;

    const float avg = 1.5f;
    NfcDesign device;
    NfcInit(343.3f / avg / 48000.0f, device);
    const NfcSetup nfc{avg, {device.baseGain[1], device.baseGain[2], device.baseGain[3], device.baseGain[4]}};

    HrtfStoreDev st{};
    SourceSetup cx{48000u, 0u, 0u, numDry, wet, 0u, Upload(env), Upload(std::vector<ResamplerConsts>{rs}), Upload(dryMap), Upload(wetMaps)};
    SourceRecord *drecs = Upload(recs);
    ParamRecord *out = nullptr;
    NfcRecord *nout = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void**>(&out), size_t{kMax} * sizeof(ParamRecord)));
    CHECK(hipMalloc(reinterpret_cast<void**>(&nout), size_t{kMax} * sizeof(NfcRecord)));
    if(!cx.slotEnv || !cx.rs || !cx.dryMap || !cx.wetMaps || !drecs) { std::fprintf(stderr, "allocation failed\n"); return 1; }
    hipStream_t s;
    hipEvent_t e0, e1;
    CHECK(hipStreamCreate(&s)); CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    const float dist0 = SourceAttenuation(recs[0].p, 44100u, lis, SourceSetup{48000u, 0u, 0u, numDry, wet, 0u, env.data(), &rs, dryMap.data(), wetMaps.data()}).distance;
    const uint32_t counts[3] = {1u, 64u, kMax};
    for(uint32_t count : counts)
        for(int which = 0; which < 2; ++which)
        {
            std::vector<float> us;
            for(int k = 0; k < 55; ++k)
            {
                if(which == 0) LaunchSourceNfc(s, cx, lis, nfc, drecs, nullptr, count, nout, e0, e1);
                else LaunchSourceParams(s, cx, st, lis, drecs, count, out, e0, e1);
                CHECK(hipGetLastError());
                CHECK(hipStreamSynchronize(s));
                float ms = 0.0f;
                CHECK(hipEventElapsedTime(&ms, e0, e1));
                if(k >= 5) us.push_back(ms * 1000.0f);
            }
            std::vector<NfcRecord> back(count);
            CHECK(hipMemcpy(back.data(), nout, size_t{count} * sizeof(NfcRecord), hipMemcpyDeviceToHost));
            std::sort(us.begin(), us.end());
            std::printf("{\"kernel\": \"%s\", \"sources\": %u, \"median_us\": %.2f, \"min_us\": %.2f, \"max_us\": %.2f, \"bytes_in\": %zu, "
                "\"bytes_out\": %zu, \"w0_0\": %.9g, \"a0_last\": %.9g, \"last_voice\": %u}\n",
                which == 0 ? "SourceNfcKernel" : "SourceParamsKernel", count, us[us.size() / 2], us.front(), us.back(),
                size_t{count} * sizeof(SourceRecord), size_t{count} * (which == 0 ? sizeof(NfcRecord) : sizeof(ParamRecord)),
                SourceNfcW0(dist0, lis.nfc_scale, avg, 48000u), back[count - 1].a0[3], back[count - 1].voice);
        }
    return 0;
}
