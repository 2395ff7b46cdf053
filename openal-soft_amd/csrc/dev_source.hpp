// The parameter stage of a mono 3D point source (FmtMono, !mPanningEnabled, spatialize mode on or auto), once, for the
// device (SourceParamsKernel, source_kernels.hip) and for the host (oalgpu_source_params_host, api_sources.hip): what
// CalcAttnVoiceParams (alc/alu.cpp:1712-2010) computes, in its operation order, and what CalcPanningAndFilters
// (:1512-1657) does with the results for this source kind.
//
//   SourceAttenuation   listener transform and normalize() (common/vecmat.h:51-65, :112-120), the seven distance models with
//                       the clamped variants' attenDistance, the per-send attenuation with RoomRolloffFactor + slot.RoomRolloff,
//                       dryAttnBase, the cone, the MinGain / MaxGain clamps, Direct.Gain / Send[i].Gain, the listener gain and the
//                       GainMixMax ceiling, air absorption and the wet path's decay (both only when distance > RefDistance),
//                       Doppler (three branches), mStep, the spread from Radius -- and CalcHrtfPanning's / CalcNormalPanning's
//                       choice of direction (below)
//   SourceFilterDesign  one of the 2 + 12 setParamsFromSlope designs (dev_design.hpp)
//   PrepareResamplerDev PrepareResampler / BsincPrepare (alu.cpp:140-281) against the table constants of ResamplerConsts
//   (HrtfBlendFor, dev_hrtf.hpp: getCoeffs' index half; PanLineGain, dev_pan.hpp: CalcDirectionCoeffs + ComputePanGains)
//
// The direction.  distance > epsilon: (x, y, z) = tosource * {XScale, YScale, ZScale}; an HRTF context gets ev =
// asin(clamp(y, -1, 1)), az = atan2(x, -z), getCoeffs(ev, az, distance * NfcScale, spread) and Hrtf.Target.Gain = DryGain.Base
// (alu.cpp:1207-1227); a dry-line context ComputePanGains of CalcDirectionCoeffs((x, y, z), spread) for the dry bus and the
// sends (:1343-1362).  A source AT the listener (normalize() returned 0 and zeroed tosource): both functions' no-distance
// branches walk the channel map, which for this source kind is MonoMap's single front position (0, 0, -1) (:1471-1473).
// CalcHrtfPanning (:1272-1310): ev = asin(0), az = atan2(0, 1), an INFINITE distance, spread as it is (spreadmult = spread for
// a 3D mono source), and the sends' gains from CalcDirectionCoeffs((0, 0, -1), spread).  CalcNormalPanning (:1413-1465): the
// dry bus and the sends get ComputePanGains of CalcDirectionCoeffs((0, 0, -1), spreadmult), spreadmult = spread again, with
// pangain = 1 (GetPanGainSelector is about mPanningEnabled sources); there is no LFE entry in MonoMap and Pairwise rendering is
// out of scope.  The spread itself is 0 or 2 pi there (alu.cpp:2002-2006: Radius > 0 = distance gives 2 pi - 0).  So the
// no-distance case differs from the other only in the direction -- the unscaled front -- and in the HRTF distance.
//
// Exactness.  mStep, the resampler's kind / m / l / filter offset and the FilterActive bits decide positions and must equal the
// reference's bit for bit: every operation up to them is +, -, *, /, sqrt and comparisons (pow, acos, asin only feed gains),
// written without contraction (the pragma below, -ffp-contract=off) and without fmaf.  In the compiled gfx950 code of
// SourceParamsKernel under the Makefile's flags every fp32 division is the correctly rounded expansion (v_div_scale_f32,
// v_rcp_f32, the v_fma_f32 refinement with denormals switched on around it by s_setreg, v_div_fmas_f32, v_div_fixup_f32) and
// every sqrtf of this file and of dev_design.hpp is the compiler's correctly rounded expansion for flushed denormals (the operand
// scaled by 2^32 below 2^-96, v_rsq_f32, s = x * r and h = r / 2 refined by three v_fma_f32 with the residual x - s * s, scaled
// back, v_cmp_class_f32 for 0 and infinity): 30 such divisions and 6 such roots, no bare v_rcp_f32 or v_sqrt_f32 on a value of
// ours (the three bare v_sqrt_f32 are inside the math library's acos / asin).  hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt holds and nothing in the flags switches it off, so the _rn intrinsics are not needed.
// Gains, HF / LF gains, the HRTF direction and the filter coefficients are within the device math library's error of glibc's,
// not bit-identical.
#pragma once
#include "kernels.hpp"
#include "dev_design.hpp"
#include "dev_pan.hpp"

#pragma clang fp contract(off)

namespace oalgpu {

// a source record as the kernel reads it: the voice, Voice::mFrequency (oalgpu_voice_desc::frequency), the VoiceProps subset
struct SourceRecord { uint32_t voice, frequency; oalgpu_source_props p; };
static_assert(sizeof(SourceRecord) == 292, "SourceRecord");

// BSincTable (core/bsinc_tables.h:11-16) of the three families without the filters, and where the families' and the cubic
// tables' filters start in the context's table blob: uploaded once per context
struct ResamplerConsts {
    struct Family { float scaleBase, scaleRange; uint32_t m[16], filterOffset[16]; } fam[3];     // bsinc12, 24, 48
    uint32_t bsincBase[3], cubicBase[2];
};

// what the stage reads of the device and the context besides the listener
struct SourceSetup {
    uint32_t sampleRate, numSends, numSlots, numDry, wetChannels, hrtf;
    const oalgpu_slot_environment *slotEnv;         // [numSlots]
    const ResamplerConsts *rs;
    const AmbiMapEntry *dryMap, *wetMaps;           // [numDry], [numSlots][wetChannels]
};

// CalcAttnVoiceParams' results, and the direction CalcPanningAndFilters pans them to
struct SourceGains {
    float dir[3];                   // the argument of CalcDirectionCoeffs (OpenAL space)
    float distance, spread;
    float hrtfEv, hrtfAz, hrtfDist; // getCoeffs' arguments (HRTF contexts)
    float dryBase, dryHF, dryLF;    // DryGain
    float wetBase[6], wetHF[6], wetLF[6];           // WetGain[i]
    int32_t sendSlot[6];            // -1: mSend[i].Buffer empty
    uint32_t step;                  // mStep
};

struct ResamplerPrep { int32_t kind, table; uint32_t m, l; float sf; uint32_t filterOffset /* in the blob */, tableOffset /* in its table */; };

// a[s] for a run-time s without indexing the array (which would move it out of the registers)
template<typename T>
__host__ __device__ __forceinline__ T Pick6(const T (&a)[6], uint32_t s)
{
    // (written out: a loop over the six entries is rewritten by the optimizer into the indexed load it stands for)
    const T a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5];
    return s == 1u ? a1 : (s == 2u ? a2 : (s == 3u ? a3 : (s == 4u ? a4 : (s == 5u ? a5 : a0))));
}

__host__ __device__ __forceinline__ float SrcLerp(float a, float b, float mu) { return a + (b - a) * mu; }                 // lerpf, common/alnumeric.h
__host__ __device__ __forceinline__ float SrcClamp(float v, float lo, float hi) { return (v < lo) ? lo : ((hi < v) ? hi : v); }   // std::clamp
__host__ __device__ __forceinline__ float SrcDot(const float *a, const float *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// al::Vector::normalize, common/vecmat.h:51-65
__host__ __device__ __forceinline__ float SrcNormalize(float *v)
{
    const float lengthSqr = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    if(lengthSqr > kFltEpsilon)
    {
        const float length = sqrtf(lengthSqr);
        const float invLength = 1.0f / length;
        v[0] *= invLength; v[1] *= invLength; v[2] *= invLength;
        return length;
    }
    v[0] = v[1] = v[2] = 0.0f;
    return 0.0f;
}

// al::Matrix * al::Vector, common/vecmat.h:112-120
__host__ __device__ __forceinline__ void SrcTransform(const float *m, const float *vec, float *out)
{
#pragma unroll
    for(int c = 0; c < 4; ++c)
        out[c] = vec[0] * m[0 * 4 + c] + vec[1] * m[1 * 4 + c] + vec[2] * m[2 * 4 + c] + vec[3] * m[3 * 4 + c];
}

__host__ __device__ __forceinline__ SourceGains SourceAttenuation(const oalgpu_source_props &p, uint32_t frequency, const oalgpu_listener_params &lis,
    const SourceSetup &cx)
{
    constexpr float kGainMixMax = 1000.0f;                  // alc/alu.h:18
    constexpr float kSpeedOfSoundMetersPerSec = 343.3f;     // core/context.h:32
    constexpr float kReverbDecayGain = 0.001f;              // core/effects/base.h:22
    constexpr float kPi = 3.14159265358979323846f;
    SourceGains g;

    // the sends' slots and room rolloff (alu.cpp:1721-1741)
    float roomRolloff[6], slotDecayTime[6], slotAirAbsorb[6];
#pragma unroll
    for(uint32_t s = 0; s < 6; ++s)
    {
        g.sendSlot[s] = -1; roomRolloff[s] = 0.0f; slotDecayTime[s] = 0.0f; slotAirAbsorb[s] = 1.0f;
        const int32_t slot = p.send[s].slot;
        if(s < cx.numSends && slot >= 0 && uint32_t(slot) < cx.numSlots && cx.slotEnv[slot].active)
        {
            g.sendSlot[s] = slot;
            roomRolloff[s] = p.room_rolloff_factor + cx.slotEnv[slot].room_rolloff;
            slotDecayTime[s] = cx.slotEnv[slot].decay_time;
            slotAirAbsorb[s] = cx.slotEnv[slot].air_absorption_gain_hf;
        }
    }

    // source -> listener space (alu.cpp:1743-1762)
    float position[4] = {p.position[0], p.position[1], p.position[2], 1.0f};
    float velocity[4] = {p.velocity[0], p.velocity[1], p.velocity[2], 0.0f};
    float direction[4] = {p.direction[0], p.direction[1], p.direction[2], 0.0f};
    if(!p.head_relative)
    {
        const float rel[4] = {position[0] - lis.position[0], position[1] - lis.position[1], position[2] - lis.position[2], 1.0f - 1.0f};
        const float vel[4] = {velocity[0], velocity[1], velocity[2], velocity[3]};
        const float dir[4] = {direction[0], direction[1], direction[2], direction[3]};
        SrcTransform(lis.matrix, rel, position);
        SrcTransform(lis.matrix, vel, velocity);
        SrcTransform(lis.matrix, dir, direction);
    }
    else
    {
        velocity[0] += lis.velocity[0]; velocity[1] += lis.velocity[1]; velocity[2] += lis.velocity[2];
    }
    float tosource[3] = {position[0], position[1], position[2]};
    const float distance = SrcNormalize(tosource);
    const bool directional = SrcNormalize(direction) > 0.0f;

    // distance attenuation (alu.cpp:1764-1851)
    const int32_t model = lis.source_distance_model ? p.distance_model : lis.distance_model;
    const bool clamped = model == OALGPU_DISTANCE_INVERSE_CLAMPED || model == OALGPU_DISTANCE_LINEAR_CLAMPED
        || model == OALGPU_DISTANCE_EXPONENT_CLAMPED;
    float attenDistance = distance;
    if(clamped)
        attenDistance = !(p.ref_distance <= p.max_distance) ? p.ref_distance : SrcClamp(distance, p.ref_distance, p.max_distance);

    g.dryBase = p.gain; g.dryHF = 1.0f; g.dryLF = 1.0f;
#pragma unroll
    for(uint32_t s = 0; s < 6; ++s) { g.wetBase[s] = p.gain; g.wetHF[s] = 1.0f; g.wetLF[s] = 1.0f; }

    float dryAttnBase = 1.0f;
    if(model == OALGPU_DISTANCE_INVERSE || model == OALGPU_DISTANCE_INVERSE_CLAMPED)
    {
        if(p.ref_distance > 0.0f)
        {
            const float dist = SrcLerp(p.ref_distance, attenDistance, p.rolloff_factor);
            if(dist > 0.0f)
            {
                dryAttnBase = p.ref_distance / dist;
                g.dryBase *= dryAttnBase;
            }
#pragma unroll
            for(uint32_t s = 0; s < 6; ++s)
            {
                const float wdist = SrcLerp(p.ref_distance, attenDistance, roomRolloff[s]);
                if(s < cx.numSends && wdist > 0.0f) g.wetBase[s] = g.wetBase[s] * (p.ref_distance / wdist);
            }
        }
    }
    else if(model == OALGPU_DISTANCE_LINEAR || model == OALGPU_DISTANCE_LINEAR_CLAMPED)
    {
        if(p.max_distance != p.ref_distance)
        {
            const float scale = (attenDistance - p.ref_distance) / (p.max_distance - p.ref_distance);
            const float a = 1.0f - scale * p.rolloff_factor;
            dryAttnBase = (a < 0.0f) ? 0.0f : a;
            g.dryBase *= dryAttnBase;
#pragma unroll
            for(uint32_t s = 0; s < 6; ++s)
            {
                const float w = 1.0f - scale * roomRolloff[s];
                if(s < cx.numSends) g.wetBase[s] = g.wetBase[s] * ((w < 0.0f) ? 0.0f : w);
            }
        }
    }
    else if(model == OALGPU_DISTANCE_EXPONENT || model == OALGPU_DISTANCE_EXPONENT_CLAMPED)
    {
        if(attenDistance > 0.0f && p.ref_distance > 0.0f)
        {
            const float distRatio = attenDistance / p.ref_distance;
            dryAttnBase = powf(distRatio, -p.rolloff_factor);
            g.dryBase *= dryAttnBase;
#pragma unroll
            for(uint32_t s = 0; s < 6; ++s)
                if(s < cx.numSends) g.wetBase[s] = g.wetBase[s] * powf(distRatio, -roomRolloff[s]);
        }
    }

    // directional sound cones (alu.cpp:1853-1882)
    float wetcone = 1.0f, wetconehf = 1.0f;
    if(directional && p.inner_angle < 360.0f)
    {
        constexpr float kRad2Deg = 57.295779513082320877f;
        const float angle = kRad2Deg * 2.0f * acosf(-SrcDot(direction, tosource)) * lis.cone_scale;
        float conegain = 1.0f, conehf = 1.0f;
        if(angle >= p.outer_angle)
        {
            conegain = p.outer_gain;
            conehf = p.outer_gain_hf;
        }
        else if(angle >= p.inner_angle)
        {
            const float scale = (angle - p.inner_angle) / (p.outer_angle - p.inner_angle);
            conegain = SrcLerp(1.0f, p.outer_gain, scale);
            conehf = SrcLerp(1.0f, p.outer_gain_hf, scale);
        }
        g.dryBase *= conegain;
        if(p.dry_gain_hf_auto) g.dryHF *= conehf;
        if(p.wet_gain_auto) wetcone = conegain;
        if(p.wet_gain_hf_auto) wetconehf = conehf;
    }

    // gain clamps, the filters' gains, the listener gain, the ceiling (alu.cpp:1884-1903)
    const float mingain = (p.max_gain < p.min_gain) ? p.max_gain : p.min_gain;
    const float maxgain = p.max_gain;
    g.dryBase = SrcClamp(g.dryBase, mingain, maxgain) * p.direct_gain;
    {
        const float x = g.dryBase * lis.gain;
        g.dryBase = (x < kGainMixMax) ? x : kGainMixMax;
    }
    g.dryHF = g.dryHF * p.direct_gain_hf;
    g.dryLF = p.direct_gain_lf;
#pragma unroll
    for(uint32_t s = 0; s < 6; ++s)
    {
        const float gain = SrcClamp(g.wetBase[s] * wetcone, mingain, maxgain) * p.send[s].gain;
        const float x = gain * lis.gain;
        g.wetBase[s] = (x < kGainMixMax) ? x : kGainMixMax;
        g.wetHF[s] = p.send[s].gain_hf * wetconehf;
        g.wetLF[s] = p.send[s].gain_lf;
    }

    // distance-based air absorption and initial send decay (alu.cpp:1905-1954)
    if(distance > p.ref_distance)
    {
        const float distanceUnits = (distance - p.ref_distance) * p.rolloff_factor;
        const float distanceMeters = distanceUnits * lis.meters_per_unit;
        const float absorb = distanceMeters * p.air_absorption_factor;
        if(absorb > kFltEpsilon) g.dryHF *= powf(lis.air_absorption_gain_hf, absorb);
        if(p.wet_gain_auto)
        {
#pragma unroll
            for(uint32_t s = 0; s < 6; ++s)
            {
                if(g.sendSlot[s] < 0 || !(slotDecayTime[s] > 0.0f)) continue;
                if(slotAirAbsorb[s] < 1.0f && absorb > kFltEpsilon) g.wetHF[s] *= powf(slotAirAbsorb[s], absorb);
                const float decayDistance = slotDecayTime[s] * kSpeedOfSoundMetersPerSec;
                const float fact = distanceMeters / decayDistance;
                const float gain = powf(kReverbDecayGain, fact) * (1.0f - dryAttnBase) + dryAttnBase;
                g.wetBase[s] *= gain;
            }
        }
    }

    // velocity-based doppler, the rates, the fixed-point step (alu.cpp:1957-1999)
    float pitch = p.pitch;
    const float dopplerFactor = p.doppler_factor * lis.doppler_factor;
    if(dopplerFactor > 0.0f)
    {
        const float vss = SrcDot(velocity, tosource) * -dopplerFactor;
        const float vls = SrcDot(lis.velocity, tosource) * -dopplerFactor;
        const float speedOfSound = lis.speed_of_sound;
        if(!(vls < speedOfSound)) pitch = 0.0f;
        else if(!(vss < speedOfSound)) pitch = __builtin_inff();
        else pitch *= (speedOfSound - vls) / (speedOfSound - vss);
    }
    pitch *= float(frequency) / float(cx.sampleRate);
    if(pitch > 10.0f) g.step = 10u << kFracBits;            // MaxPitch, core/voice.h:33
    else
    {
        const uint32_t st = fastf2u(pitch * float(kFracOne));
        g.step = st > 1u ? st : 1u;
    }

    // the spread of a source with a radius (alu.cpp:2002-2006)
    float spread = 0.0f;
    if(p.radius > distance) spread = kPi * 2.0f - distance / p.radius * kPi;
    else if(distance > 0.0f) spread = asinf(p.radius / distance) * 2.0f;
    g.distance = distance; g.spread = spread;

    // CalcPanningAndFilters' direction for this source kind (see the head of this file)
    if(distance > kFltEpsilon)
    {
        g.dir[0] = tosource[0] * lis.xyz_scale[0]; g.dir[1] = tosource[1] * lis.xyz_scale[1]; g.dir[2] = tosource[2] * lis.xyz_scale[2];
        g.hrtfDist = distance * lis.nfc_scale;
    }
    else
    {
        g.dir[0] = 0.0f; g.dir[1] = 0.0f; g.dir[2] = -1.0f;
        g.hrtfDist = __builtin_inff();
    }
    g.hrtfEv = 0.0f; g.hrtfAz = 0.0f;
    if(cx.hrtf)
    {
        g.hrtfEv = asinf(SrcClamp(g.dir[1], -1.0f, 1.0f));
        g.hrtfAz = atan2f(g.dir[0], -g.dir[2]);
    }
    return g;
}

// FilterActive of the direct path and of the sends (alu.cpp:1624-1626, :1643-1645) as ParamRecord::flags keeps them
__host__ __device__ __forceinline__ uint32_t SourceFilterFlags(const SourceGains &g, uint32_t numSends)
{
    uint32_t flags = (g.dryHF != 1.0f || g.dryLF != 1.0f) ? uint32_t(kFlagDirectFilter) : 0u;
#pragma unroll
    for(uint32_t s = 0; s < 6; ++s)
        if(s < numSends && (g.wetHF[s] != 1.0f || g.wetLF[s] != 1.0f)) flags |= 1u << (kFlagSendFilterShift + s);
    return flags;
}

// Filter k of a record, in ParamRecord's order -- 0: dirLp, 1: dirHp, 2 + s: sendLp[s], 8 + s: sendHp[s] -- designed as
// CalcPanningAndFilters does (alu.cpp:1619-1656): the "low pass" is a high shelf at HFReference / rate with the HF gain, the
// "high pass" a low shelf at LFReference / rate with the LF gain, slope 1.  Sends the device does not have stay zero.
__host__ __device__ __forceinline__ void SourceFilterDesign(uint32_t k, const oalgpu_source_props &p, const SourceGains &g, const SourceSetup &cx, float c[5])
{
    const float invSampleRate = 1.0f / float(cx.sampleRate);
    const bool direct = k < 2u;
    const bool high = k == 0u || (k >= 2u && k < 8u);
    const uint32_t s = direct ? 0u : (k < 8u ? k - 2u : k - 8u);
    c[0] = c[1] = c[2] = c[3] = c[4] = 0.0f;
    if(!direct && s >= cx.numSends) return;
    const float reference = direct ? (high ? p.direct_hf_reference : p.direct_lf_reference)
        : (high ? p.send[s].hf_reference : p.send[s].lf_reference);
    const float gain = direct ? (high ? g.dryHF : g.dryLF) : (high ? Pick6(g.wetHF, s) : Pick6(g.wetLF, s));
    DesignBiquadFromSlope(high ? OALGPU_BIQUAD_HIGHSHELF : OALGPU_BIQUAD_LOWSHELF, reference * invSampleRate, gain, 1.0f, c);
}

// PrepareResampler + BsincPrepare (alu.cpp:140-281; host/params.cpp's PrepareResampler on the table constants)
__host__ __device__ __forceinline__ ResamplerPrep PrepareResamplerDev(const ResamplerConsts &rs, int resampler, uint32_t increment)
{
    ResamplerPrep r{};
    switch(resampler)
    {
    case OALGPU_RESAMPLER_POINT: r.kind = 0; return r;
    case OALGPU_RESAMPLER_LINEAR: r.kind = 1; return r;
    case OALGPU_RESAMPLER_SPLINE: r.kind = 2; r.table = 0; r.filterOffset = rs.cubicBase[0]; return r;
    case OALGPU_RESAMPLER_GAUSSIAN: r.kind = 2; r.table = 1; r.filterOffset = rs.cubicBase[1]; return r;
    default: break;
    }
    const bool fastOnly = resampler == OALGPU_RESAMPLER_FAST_BSINC12 || resampler == OALGPU_RESAMPLER_FAST_BSINC24
        || resampler == OALGPU_RESAMPLER_FAST_BSINC48;
    const uint32_t f = (resampler == OALGPU_RESAMPLER_FAST_BSINC12 || resampler == OALGPU_RESAMPLER_BSINC12) ? 0u
        : ((resampler == OALGPU_RESAMPLER_FAST_BSINC24 || resampler == OALGPU_RESAMPLER_BSINC24) ? 1u : 2u);
    uint32_t si = 15;
    float sf = 0.0f;
    if(increment > kFracOne) BsincScale(rs.fam[f].scaleBase, rs.fam[f].scaleRange, increment, si, sf);
    si = si < 15u ? si : 15u;                               // (never above 15 for a step that is a number: the guard of the table reads)
    r.kind = (!fastOnly && increment > kFracOne) ? 4 : 3;
    r.table = f == 0u ? 12 : (f == 1u ? 24 : 48);
    r.sf = sf;
    r.m = rs.fam[f].m[si];
    r.l = r.m / 2u - 1u;
    r.tableOffset = rs.fam[f].filterOffset[si];
    r.filterOffset = rs.bsincBase[f] + r.tableOffset;
    return r;
}

// ---- launcher (source_kernels.hip): `count` source records -> `count` ParamRecords, one wavefront each; evStart / evStop: events
// bound to the dispatch (null: none) ----
void LaunchSourceParams(hipStream_t s, const SourceSetup &cx, const HrtfStoreDev &st, const oalgpu_listener_params &listener,
    const SourceRecord *recs, uint32_t count, ParamRecord *out, hipEvent_t evStart = nullptr, hipEvent_t evStop = nullptr);

} // namespace oalgpu
