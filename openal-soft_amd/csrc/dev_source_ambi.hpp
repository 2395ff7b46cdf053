// The parameter stage of B-Format sources (FmtBFormat2D / FmtBFormat3D, orders 1..4), once, for the device (AmbiParamsKernel,
// source_ambi_kernels.hip) and for the host (oalgpu_ambi_source_params_host, api_sources.hip): CalcAmbisonicPanning
// (alc/alu.cpp:911-1076) with AmbiRotator (:799-888) and UpsampleBFormatTransform (:457-477), on dry-line contexts.
//
//   the route              a B-Format source is never "mono 3D" (alu.cpp:2024-2030): spatialize OFF or AUTO takes
//                          dev_source_channels.hpp's SourceNonAttenuation (it pans with distance 0), ON dev_source.hpp's
//                          SourceAttenuation; both called, not restated.  Filters, mStep, the resampler, FilterActive and the send
//                          slots are the source's, equal in every channel voice
//   AmbiCoverage           1 when !(distance > epsilon), else inv_pi * 0.5 * spread (:947-948)
//   AmbiOrientation        N and V normalised, through the listener matrix unless head-relative, U = N x V normalised, the
//                          zeroth- and first-order block of the rotation (:976-998)
//   AmbiRotatorElement     one element of band l >= 2 from band l - 1 and band 1, its u / v / w terms skipped when their
//                          constant is zero, in the order u, v, w (:857-887).  The constants (RotatorCoeffs, :738-792) are
//                          computed in double and narrowed by the host at library start (FillAmbiRotatorCoeffs below, which
//                          also says why v of m = 0 is the recurrence's -sqrt((l - 1) l / (2 denom)), not the reference's)
//   AmbiUpsampleEntry      out[i][j] = sum over k, ascending, of rot[k][j] * up[i][k] + out, zero entries included (:467-475)
//   AmbiChannelCoeff       mix[acn][j] * (scales[acn] * coverage) + (c == 0 ? panned[j] * ((1 - coverage) * scales[0]) : 0)
//   AmbiLineGain           one line of ComputePanGains over such coefficients (core/mixer.cpp:92-102)
//
// A source without coverage (distance > epsilon, spread 0) pans its channel 0 alone: CalcDirectionCoeffs(pos, 0) under Base *
// scales[0] (:959-970); the other channel voices get zero targets.  Only + - * / sqrt and comparisons lie between the source's
// orientation and the mix matrix, written without contraction and without fmaf (dev_source.hpp, "Exactness"): host and device
// agree bit for bit on the matrix, and on every line gain of the non-attenuated route.
#pragma once
#include "dev_source_channels.hpp"

#pragma clang fp contract(off)

namespace oalgpu {

constexpr uint32_t kAmbiMax = OALGPU_MAX_AMBI_CHANNELS;          // the matrices are kAmbiMax x kAmbiMax, row-major
constexpr uint32_t kAmbiMatrix = kAmbiMax * kAmbiMax;
constexpr uint32_t kRotatorCoeffs = 25u + 49u + 81u;             // CalcRotatorSize(4): the bands 2, 3, 4

// an ambisonic source as the kernel reads it.  The host resolves the layout and the scaling (GetAmbiLayout / GetAmbi2DLayout,
// GetAmbiScales) into acn[c] = index_map[c] and scale[c] = scales[acn[c]], and the upsampler the device order asks for into its
// place in the context's store (upRows 0: none, the mix matrix is the rotation)
struct AmbiSourceRecord {
    uint32_t frequency, present, outBase;       // present: bit c = channel c has a voice
    int32_t spatialize;
    uint32_t channels;                          // (order + 1)^2, or 2 order + 1 for a 2D format
    uint32_t upRows, upOffset;                  // the upsampler: rows, and its first float in AmbiSetup::upsamplers
    float scale0;                               // scales[0]
    float orientAt[3], orientUp[3];
    uint8_t acn[28];
    float scale[kAmbiMax];
    uint32_t voices[kAmbiMax];
    oalgpu_source_props p;
};
static_assert(sizeof(AmbiSourceRecord) == 32 + 24 + 28 + 100 + 100 + 284, "AmbiSourceRecord");

// what the stage reads of the device besides SourceSetup: DeviceBase::mAmbiOrder, RotatorCoeffArray as {u, v, w} triples in
// its order (band, n, m), the upsamplers the context was given
struct AmbiSetup { uint32_t order; const float *rotCoeffs, *upsamplers; };

__host__ __device__ __forceinline__ uint32_t AmbiChannelsOfOrder(uint32_t order) { return (order + 1u) * (order + 1u); }

__host__ __device__ __forceinline__ float AmbiCoverage(float distance, float spread)
{
    return !(distance > kFltEpsilon) ? 1.0f : (0.318309886183790671538f * 0.5f * spread);
}

// what CalcAmbisonicPanning receives as (xpos, ypos, zpos): SourceGains::dir, except on the attenuated route at the listener,
// where CalcAttnVoiceParams hands the zeroed ToSource times the scales down (alu.cpp:2008-2009) and not MonoMap's front.  (The
// zeros are taken as +0: a negative XScale / YScale / ZScale would make them -0 in the reference, which shows in nothing but the
// sign of a zero coefficient: the panned share is multiplied by 1 - coverage = 0 there.)
__host__ __device__ __forceinline__ void AmbiPanPosition(const SourceGains &g, bool attenuated, float (&pos)[3])
{
    const bool atListener = attenuated && !(g.distance > kFltEpsilon);
    pos[0] = atListener ? 0.0f : g.dir[0]; pos[1] = atListener ? 0.0f : g.dir[1]; pos[2] = atListener ? 0.0f : g.dir[2];
}

// CalcVoiceParams' route for a B-Format source (alu.cpp:2024-2030): true = CalcAttnVoiceParams
__host__ __device__ __forceinline__ bool AmbiSourceRoute(int32_t spatialize) { return spatialize == OALGPU_SPATIALIZE_ON; }

// the first-order block of shrot (alu.cpp:976-998) as nine floats: rows 1..3, columns 1..3
__host__ __device__ __forceinline__ void AmbiOrientation(const float (&at)[3], const float (&up)[3], int32_t headRelative,
    const oalgpu_listener_params &lis, float (&block)[9])
{
    float N[4] = {at[0], at[1], at[2], 0.0f};
    SrcNormalize(N);
    float V[4] = {up[0], up[1], up[2], 0.0f};
    SrcNormalize(V);
    if(!headRelative)
    {
        const float n[4] = {N[0], N[1], N[2], N[3]}, v[4] = {V[0], V[1], V[2], V[3]};
        SrcTransform(lis.matrix, n, N);
        SrcTransform(lis.matrix, v, V);
    }
    // al::Vector::cross_product, common/vecmat.h
    float U[3] = {N[1] * V[2] - N[2] * V[1], N[2] * V[0] - N[0] * V[2], N[0] * V[1] - N[1] * V[0]};
    SrcNormalize(U);
    block[0] = U[0]; block[1] = -U[1]; block[2] = U[2];
    block[3] = -V[0]; block[4] = V[1]; block[5] = -V[2];
    block[6] = -N[0]; block[7] = N[1]; block[8] = -N[2];
}

// AmbiRotator's P (alu.cpp:804-819); R: the matrix, kAmbiMax floats a row
__host__ __device__ __forceinline__ float AmbiRotP(const float *R, int i, int l, int a, int n, int lastBase)
{
    const int ip2 = i + 2;
    const float ri1 = R[3 * int(kAmbiMax) + ip2], rim1 = R[1 * int(kAmbiMax) + ip2], ri0 = R[2 * int(kAmbiMax) + ip2];
    const int lm1 = l - 1;
    const int x = lastBase + lm1 + a;
    if(n == -l) return ri1 * R[lastBase * int(kAmbiMax) + x] + rim1 * R[(lastBase + lm1 * 2) * int(kAmbiMax) + x];
    if(n == l) return ri1 * R[(lastBase + lm1 * 2) * int(kAmbiMax) + x] - rim1 * R[lastBase * int(kAmbiMax) + x];
    return ri0 * R[(lastBase + lm1 + n) * int(kAmbiMax) + x];
}

// matrix[base + l + n][base + l + m] of band l (2..4; base = l * l, lastBase = (l - 1)^2) from the bands below it, alu.cpp:869-879;
// uvw: the element's {u, v, w}
__host__ __device__ __forceinline__ float AmbiRotatorElement(const float *R, const float *uvw, int l, int n, int m)
{
    constexpr float kSqrt2 = 1.41421356237309504880f;
    const int lastBase = (l - 1) * (l - 1);
    const float u = uvw[0], v = uvw[1], w = uvw[2];
    float r = 0.0f;
    if(u != 0.0f) r += u * AmbiRotP(R, 0, l, m, n, lastBase);
    if(v != 0.0f)
    {
        float V;
        if(m > 0)
        {
            const float p0 = AmbiRotP(R, 1, l, m - 1, n, lastBase), p1 = AmbiRotP(R, -1, l, -m + 1, n, lastBase);
            V = (m == 1) ? p0 * kSqrt2 : (p0 - p1);
        }
        else
        {
            const float p0 = AmbiRotP(R, 1, l, m + 1, n, lastBase), p1 = AmbiRotP(R, -1, l, -m - 1, n, lastBase);
            V = (m == -1) ? p1 * kSqrt2 : (p0 + p1);
        }
        r += v * V;
    }
    if(w != 0.0f)
    {
        float W;
        if(m > 0) W = AmbiRotP(R, 1, l, m + 1, n, lastBase) + AmbiRotP(R, -1, l, -m - 1, n, lastBase);
        else W = AmbiRotP(R, 1, l, m - 1, n, lastBase) - AmbiRotP(R, -1, l, -m + 1, n, lastBase);
        r += w * W;
    }
    return r;
}

// RotatorCoeffs (alu.cpp:738-792) for the host: the {u, v, w} of every element of the bands 2..4 in the order (band, n, m), in
// double, narrowed, into out[kRotatorCoeffs * 3] (the library at its start, tools/ubench_source_ambi.hip).
// ONE constant is not the reference's: v of m = 0.  Ivanic and Ruedenberg's Table I has v = 1/2 sqrt((1 + delta_m0) (l + |m| - 1)
// (l + |m|) / denom) (1 - 2 delta_m0), which for m = 0 is -sqrt((l - 1) l / (2 denom)); the reference multiplies by (1 + delta_m0)
// OUTSIDE the root (its comment at :762-763, its code at :774) and gets -sqrt((l - 1) l / denom).  With that the m = 0 column of
// every band, and through the recurrence the columns |m| <= l - 2 of the bands above, are not a rotation's (the matrix is off
// orthogonality by up to 0.5); with the table's value it is one to float32 rounding (tests/test_ambi_sources_host.py).  A 2D
// device reads only the columns |m| = l, which do not depend on the constant.
inline void FillAmbiRotatorCoeffs(float *out)
{
    for(int l = 2; l <= OALGPU_MAX_AMBI_ORDER; ++l)
        for(int n = -l; n <= l; ++n)
            for(int m = -l; m <= l; ++m)
            {
                const double denom = double((n == l || n == -l) ? (2 * l) * (2 * l - 1) : (l * l - n * n));
                const int abs_m = m < 0 ? -m : m;
                *out++ = float(__builtin_sqrt((l * l - m * m) / denom));
                *out++ = m == 0 ? float(__builtin_sqrt(2.0 * ((l - 1) * l) / denom) * -0.5)
                    : float(__builtin_sqrt((l + abs_m - 1) * (l + abs_m) / denom) * 0.5);
                *out++ = m == 0 ? 0.0f : float(__builtin_sqrt((l - abs_m - 1) * (l - abs_m) / denom) * -0.5);
            }
}

// where band l's constants start in RotatorCoeffArray (triples)
__host__ __device__ __forceinline__ uint32_t AmbiRotatorBandStart(uint32_t l) { return l == 2u ? 0u : (l == 3u ? 25u : 74u); }

// UpsampleBFormatTransform's output[i][j] (alu.cpp:465-476); up: row i of the upsampler; channels = AmbiChannelsFromOrder(device order)
__host__ __device__ __forceinline__ float AmbiUpsampleEntry(const float *R, const float *up, uint32_t j, uint32_t channels)
{
    float dst = 0.0f;
    for(uint32_t k = 0; k < channels; ++k) dst = R[k * kAmbiMax + j] * up[k] + dst;
    return dst;
}

// coeffs[j] of channel c (alu.cpp:1049-1062): mixval = mixmatrix[acn][j], pannedTerm = the panned W's share (channel 0) or 0
__host__ __device__ __forceinline__ float AmbiChannelCoeff(float mixval, float scale, float pannedTerm) { return mixval * scale + pannedTerm; }

// gains[line] of ComputePanGains for the line whose AmbiMap entry has `scale`
__host__ __device__ __forceinline__ float AmbiLineGain(float scale, float coeff, float ingain) { return scale * coeff * ingain; }

// ---- launchers (source_ambi_kernels.hip) ----
// `count` ambisonic sources -> the ParamRecords of their channel voices at out[rec.outBase ...] (the channels with a voice, in
// channel order), one 64-lane workgroup per source; evStart / evStop: events bound to the dispatch (null: none)
void LaunchAmbiParams(hipStream_t s, const SourceSetup &cx, const AmbiSetup &ambi, const oalgpu_listener_params &listener,
    const AmbiSourceRecord *recs, uint32_t count, ParamRecord *out, hipEvent_t evStart = nullptr, hipEvent_t evStop = nullptr);

} // namespace oalgpu
