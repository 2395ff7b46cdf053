// C-ABI of the small EffectStates (include/oalgpu.h: oalgpu_effect_*): deviceUpdate / update as the reference does
// them on its mixer thread with libm -- biquad design, the echo's delays, the modulator's carrier period -- and the
// scalar bookkeeping process() performs (delay-line offset, carrier index); the block itself is one launch
// (effects_kernels.hip, effects2_kernels.hip).  Each kind is described once: what it owns in oalgpu_effect, its
// DeviceUpdate / Update / Begin / Advance functions, and its row of kKinds, which every entry point dispatches through.
#include "api_util.hpp"
#include "kernels.hpp"
#include "../host/params.hpp"
#include "../host/tables.hpp"

#include <cmath>
#include <memory>
#include <vector>

using namespace oalgpu;

struct FxHop { uint32_t count, pos; };   // the fill counter of a shifter's STFT (mCount / mPos), moved on by AdvanceHop

struct oalgpu_effect {
    int device{0}, kind{0};
    uint32_t sampleRate{48000}, numIn{1}, nlines{1};
    bool updated{false};
    DevBuf<FxState> st;                  // equalizer .. compressor (effects_kernels.hip)
    DevBuf<Fx2State> st2;                // chorus .. pitch shifter (effects2_kernels.hip)
    DevBuf<float> tgtGains, upTgt, hostIn, hostOut;
    FxLaunch F{}; Fx2Launch G{};
    // ---- what each kind owns besides ----
    struct { uint32_t index{0}, range{1}; } modulator;                   // ModulatorState::mIndex / mRange (modulator.cpp:75-77)
    struct { uint32_t offset{0}; DevBuf<float> line; } echo;             // EchoState::mOffset (echo.cpp:55)
    // ChorusState::mOffset / mLfoOffset / mLfoRange / mLfoDisp (chorus.cpp:83-88)
    struct { uint32_t offset{0}, lfoOffset{0}, lfoRange{1}, lfoDisp{0}; DevBuf<float> line, cubic; } chorus;
    struct { uint32_t index{0}; } vmorpher;                              // VmorpherState::mIndex (vmorpher.cpp:152)
    struct {                                                             // FshifterState::mCount / mPos / mChans[c].mPhase (fshifter.cpp:100-113)
        FxHop hop{0, 1024 - 256};
        uint32_t phase4[4]{};
        DevBuf<double> in; DevBuf<FsPair> outFifo, accum, outdata, tw, phase; DevBuf<float> window;
    } fshifter;
    struct {                                                             // PshifterState::mCount / mPos (pshifter.cpp:86-87)
        FxHop hop{0, 1024 - 128};
        uint32_t parity{0};
        DevBuf<float> ring, phase, accum, outFifo, rows, tw, window;     // ring / phase: two copies, read [parity], written [parity ^ 1]
    } pshifter;
};

namespace {

constexpr double kPi = 3.14159265358979323846; constexpr float kPiF = 3.14159265358979323846f;

template<typename T>
int UploadAt(void *base, size_t offset, const T *src, size_t count)
{ HIP_TRY(hipMemcpy(static_cast<char*>(base) + offset, src, count * sizeof(T), hipMemcpyHostToDevice)); return OALGPU_OK; }

int UploadBiquad(oalgpu_effect *e, uint32_t chan, uint32_t which, const float c[5])
{   // copyParamsFrom / setParams: the coefficients change, the filter's history stays
    return UploadAt(e->st.p, offsetof(FxState, bq) + (size_t{chan} * 4 + which) * sizeof(BiquadState) + offsetof(BiquadState, b0), c, 5);
}

uint32_t NextPow2(uint32_t v) { uint32_t p = 1; while(p < v) p <<= 1; return p; }
// float2int / float2uint (common/alnumeric.h): truncation; fastf2u: round to nearest even (cvtss2si)
int32_t TruncI(float f) { return static_cast<int32_t>(f); }
uint32_t TruncU(float f) { return static_cast<uint32_t>(static_cast<int64_t>(f)); }
uint32_t RoundU(float f) { return static_cast<uint32_t>(static_cast<int32_t>(std::lrintf(f))); }

// gHannWindow<1024>, common/hann_window.hpp: sin^2 through double, mirrored
int UploadHannWindow1024(DevBuf<float> &window)
{
    std::vector<float> win(1024);
    const double scale = kPi / double(1024 + 1);
    for(uint32_t i = 0; i < 512; ++i)
    {
        const double v = std::sin((i + 1.0) * scale);
        win[i] = win[1023 - i] = static_cast<float>(v * v);
    }
    HIP_TRY(window.alloc(win.size())); HIP_TRY(window.upload(win.data(), win.size()));
    return OALGPU_OK;
}

// `n` more samples into an STFT that transforms whenever `hop` have come in and then moves on in its 1024-sample FIFO
void AdvanceHop(FxHop &h, uint32_t hop, uint32_t n)
{
    for(uint32_t base = 0; base < n;)
    {
        const uint32_t todo = std::min(hop - h.count, n - base);
        h.count += todo; base += todo;
        if(h.count < hop) break;
        h.count = 0; h.pos = (h.pos + hop) & 1023u;
    }
}

#pragma clang fp contract(off)
// cos(pi / 2^i), sin(pi / 2^i) correctly rounded to double (tools/gen_fft_twiddle_roots.py derives them with 60-digit
// arithmetic): what complex_fft's table gArgAngle (common/alcomplex.cpp:84-99) holds
constexpr double kFftRoots[10][2] = {
    {-0x1.0000000000000p+0, 0x0.0p+0},
    {0x0.0p+0, 0x1.0000000000000p+0},
    {0x1.6a09e667f3bcdp-1, 0x1.6a09e667f3bcdp-1},
    {0x1.d906bcf328d46p-1, 0x1.87de2a6aea963p-2},
    {0x1.f6297cff75cb0p-1, 0x1.8f8b83c69a60bp-3},
    {0x1.fd88da3d12526p-1, 0x1.917a6bc29b42cp-4},
    {0x1.ff621e3796d7ep-1, 0x1.91f65f10dd814p-5},
    {0x1.ffd886084cd0dp-1, 0x1.92155f7a3667ep-6},
    {0x1.fff62169b92dbp-1, 0x1.921d1fcdec784p-7},
    {0x1.fffd8858e8a92p-1, 0x1.921f0fe670071p-8},
};

// the twiddle factors complex_fft (common/alcomplex.cpp:105-148) runs through: stage i starts from
// w = polar(1, pi / 2^i) and multiplies u by w once per j
void BuildTwiddles(std::vector<FsPair> &tw)
{
    tw.assign(1024, FsPair{1.0, 0.0});
    for(uint32_t i = 0; i < 10; ++i)
    {
        const uint32_t step2 = 1u << i;
        const FsPair w{kFftRoots[i][0], kFftRoots[i][1]};
        FsPair u = w;
        for(uint32_t j = 1; j < step2; ++j)
        {
            tw[step2 + j] = u;
            const double re = u.x * w.x - u.y * w.y, im = u.x * w.y + u.y * w.x;
            u = FsPair{re, im};
        }
    }
}

// ---- Per kind: the functions of KindInfo (below), named after the reference's members ----

int EqualizerUpdate(oalgpu_effect *e, float rate, const void *props, const float*)
{   // EqualizerState::update, equalizer.cpp:115-165
    const auto &p = *static_cast<const oalgpu_equalizer_props*>(props);
    float c[4][5];
    DesignBiquadFromSlope(OALGPU_BIQUAD_LOWSHELF, p.low_cutoff / rate, std::sqrt(p.low_gain), 0.75f, c[0]);
    DesignBiquadFromBandwidth(OALGPU_BIQUAD_PEAKING, p.mid1_center / rate, std::sqrt(p.mid1_gain), p.mid1_width, c[1]);
    DesignBiquadFromBandwidth(OALGPU_BIQUAD_PEAKING, p.mid2_center / rate, std::sqrt(p.mid2_gain), p.mid2_width, c[2]);
    DesignBiquadFromSlope(OALGPU_BIQUAD_HIGHSHELF, p.high_cutoff / rate, std::sqrt(p.high_gain), 0.75f, c[3]);
    for(uint32_t ch = 0; ch < e->numIn; ++ch)
        for(uint32_t k = 0; k < 4; ++k)
            if(int rc = UploadBiquad(e, ch, k, c[k])) return rc;
    return OALGPU_OK;
}

int ModulatorUpdate(oalgpu_effect *e, float rate, const void *props, const float*)
{   // ModulatorState::update, modulator.cpp:103-163
    const auto &p = *static_cast<const oalgpu_modulator_props*>(props);
    FxLaunch &F = e->F; auto &m = e->modulator;
    const float perCycle = p.frequency > 0.0f ? rate / p.frequency + 0.5f : 1.0f;
    const uint32_t range = uint32_t(std::min(std::max(perCycle, 1.0f), rate));
    m.index = uint32_t(uint64_t{m.index} * range / m.range);
    m.range = range;
    F.modScale = 0.0f; F.modWave = 0;
    if(m.range == 1) {}
    else if(p.waveform == OALGPU_MODULATOR_SINUSOID) { F.modScale = kPiF * 2.0f / float(m.range); F.modWave = 1; }
    else if(p.waveform == OALGPU_MODULATOR_SAWTOOTH) { F.modScale = 2.0f / float(m.range - 1u); F.modWave = 2; }
    else
    {
        m.range = (m.range + 1u) & ~1u;
        F.modScale = 1.0f / float(m.range - 1u); F.modWave = 3;
    }
    const float f0norm = std::min(std::max(p.high_pass_cutoff / rate, 1.0f / 512.0f), 0.49f);
    float c[5];
    DesignBiquadFromBandwidth(OALGPU_BIQUAD_HIGHPASS, f0norm, 1.0f, 0.75f, c);
    for(uint32_t ch = 0; ch < e->numIn; ++ch)
        if(int rc = UploadBiquad(e, ch, 0, c)) return rc;
    return OALGPU_OK;
}
int ModulatorBegin(oalgpu_effect *e, uint32_t&) { e->F.modIndex = e->modulator.index; e->F.modRange = e->modulator.range; return OALGPU_OK; }
void ModulatorAdvance(oalgpu_effect *e, uint32_t n)           // modulator.cpp:176-189
{ if(e->modulator.range > 1) e->modulator.index = (e->modulator.index + n) % e->modulator.range; }

int EchoDeviceUpdate(oalgpu_effect *e, FxState&)
{   // EchoState::deviceUpdate, echo.cpp:77-91: EchoMaxDelay 0.207 s + EchoMaxLRDelay 0.404 s, next power of two
    const float f = float(e->sampleRate);
    const uint32_t len = NextPow2(uint32_t(0.207f * f + 0.5f) + uint32_t(0.404f * f + 0.5f));
    HIP_TRY(e->echo.line.alloc_zero(len));
    e->F.delay = e->echo.line.p; e->F.delayMask = len - 1u;
    return OALGPU_OK;
}
int EchoUpdate(oalgpu_effect *e, float rate, const void *props, const float *gains)
{   // EchoState::update, echo.cpp:93-117 (the two taps' panned gains come from the caller)
    const auto &p = *static_cast<const oalgpu_echo_props*>(props);
    FxLaunch &F = e->F;
    F.tap[0] = std::max(uint32_t(std::round(p.delay * rate)), 1u);
    F.tap[1] = uint32_t(std::round(p.lr_delay * rate)) + F.tap[0];
    if(F.tap[1] > F.delayMask) return Fail(OALGPU_ERR_INVALID, "oalgpu_effect_update: echo delays beyond AL_ECHO_MAX_DELAY + AL_ECHO_MAX_LRDELAY");
    const float gainhf = std::max(1.0f - p.damping, 0.0625f);
    float c[5];
    DesignBiquadFromSlope(OALGPU_BIQUAD_HIGHSHELF, 5000.0f / rate, gainhf, 1.0f, c);
    if(int rc = UploadBiquad(e, 0, 0, c)) return rc;
    F.feedGain = p.feedback;
    HIP_TRY(e->tgtGains.upload(gains, size_t{2} * e->nlines));
    return OALGPU_OK;
}
int EchoBegin(oalgpu_effect *e, uint32_t&) { e->F.offset = e->echo.offset; return OALGPU_OK; }
void EchoAdvance(oalgpu_effect *e, uint32_t n) { e->echo.offset = (e->echo.offset + n) & e->F.delayMask; }      // echo.cpp:127-157

// DedicatedState::update, dedicated.cpp:66-100: the gains of the target line(s), resolved by the caller
int DedicatedUpdate(oalgpu_effect *e, float, const void*, const float *gains) { HIP_TRY(e->tgtGains.upload(gains, e->nlines)); return OALGPU_OK; }

int CompressorDeviceUpdate(oalgpu_effect *e, FxState &fresh)
{   // CompressorState::deviceUpdate, compressor.cpp:87-101: 100 ms from 0.5 to 2, 200 ms back; mEnvFollower = 1
    e->F.attackMult = std::pow(2.0f / 0.5f, 1.0f / (float(e->sampleRate) * 0.1f));
    e->F.releaseMult = std::pow(0.5f / 2.0f, 1.0f / (float(e->sampleRate) * 0.2f));
    fresh.env = 1.0f;
    return OALGPU_OK;
}
int CompressorUpdate(oalgpu_effect *e, float, const void *props, const float*)
{ e->F.compOn = static_cast<const oalgpu_compressor_props*>(props)->on_off ? 1 : 0; return OALGPU_OK; }

int ChorusDeviceUpdate(oalgpu_effect *e, FxState&)
{   // ChorusState::deviceUpdate, chorus.cpp:129-163: four lines of NextPowerOf2(2 * max(ChorusMaxDelay, FlangerMaxDelay) * rate + 1)
    auto &ch = e->chorus;
    const uint32_t len = NextPow2(TruncU(0.016f * 2.0f * float(e->sampleRate)) + 1u);
    HIP_TRY(ch.line.alloc_zero(size_t{len} * 4));
    HIP_TRY(ch.cubic.alloc(kFineCubicSteps * 2 + 1)); HIP_TRY(ch.cubic.upload(GetFineCubicFilter(), kFineCubicSteps * 2 + 1));
    e->G.delay = ch.line.p; e->G.delayMask = len - 1u; e->G.cubic = ch.cubic.p;
    return OALGPU_OK;
}
int ChorusUpdate(oalgpu_effect *e, float rate, const void *props, const float*)
{   // ChorusState::update, chorus.cpp:165-251
    const auto &p = *static_cast<const oalgpu_chorus_props*>(props);
    Fx2Launch &G = e->G; auto &ch = e->chorus;
    const int32_t mindelay = 24 << 8;                       // MaxResamplerEdge << gCubicTable.sTableBits
    const float stepscale = rate * 256.0f;
    G.chWave = p.waveform;
    G.chDelay = std::max(TruncI(std::round(p.delay * stepscale)), mindelay);
    G.chDepth = std::min(float(G.chDelay) * p.depth, float(G.chDelay - mindelay));
    G.chFeedback = p.feedback;
    if(!(p.rate > 0.0f)) { ch.lfoOffset = 0; ch.lfoRange = 1; G.lfoScale = 0.0f; ch.lfoDisp = 0; }
    else
    {
        const int32_t rangeLimit = 2147483647 / 360 - 180;
        const float range = std::round(rate / p.rate);
        const uint32_t lfoRange = TruncU(std::min(range, float(rangeLimit)));
        ch.lfoOffset = ch.lfoOffset * lfoRange / ch.lfoRange;
        ch.lfoRange = lfoRange;
        G.lfoScale = (p.waveform == OALGPU_CHORUS_TRIANGLE) ? 4.0f / float(lfoRange)
            : kPiF * 2.0f / float(lfoRange);
        int32_t phase = p.phase;
        if(phase < 0) phase += 360;
        ch.lfoDisp = (lfoRange * uint32_t(phase) + 180u) / 360u;
    }
    G.lfoRange = ch.lfoRange;
    G.chAvgDelay = (uint32_t(G.chDelay) + 32768u) >> 16;         // (mDelay + MixerFracHalf) >> MixerFracBits
    // how far behind the write position a tap or the feedback reads
    const uint32_t maxTap = (uint32_t(G.chDelay) + uint32_t(std::ceil(G.chDepth)) + 1u) >> 8;
    G.chHist = std::max(maxTap + 3u, G.chAvgDelay);
    if(G.chHist > G.delayMask) return Fail(OALGPU_ERR_INVALID, "oalgpu_effect_update: chorus delay beyond the delay line");
    return OALGPU_OK;
}
int ChorusBegin(oalgpu_effect *e, uint32_t &lds)
{
    Fx2Launch &G = e->G; const auto &ch = e->chorus;
    G.offset = ch.offset;
    G.lfoStart[0] = ch.lfoOffset;
    G.lfoStart[1] = (ch.lfoOffset + ch.lfoDisp) % ch.lfoRange;
    lds = (6u * OALGPU_BUFFER_LINE_SIZE + G.chHist + OALGPU_BUFFER_LINE_SIZE) * sizeof(float);
    if(lds > 65536u) return Fail(OALGPU_ERR_INVALID, "oalgpu_effect_process: chorus delay too long for the workgroup's LDS");
    return OALGPU_OK;
}
void ChorusAdvance(oalgpu_effect *e, uint32_t n)              // chorus.cpp:283,391
{ e->chorus.offset += n; e->chorus.lfoOffset = (e->chorus.lfoOffset + n) % e->chorus.lfoRange; }

int DistortionDeviceUpdate(oalgpu_effect *e, FxState&)
{   // mChans[c].mLowpass / mBandpass start as the identity
    BiquadState ident{}; ident.b0 = 1.0f;
    BiquadState eight[8]; for(auto &b : eight) b = ident;
    return UploadAt(e->st2.p, offsetof(Fx2State, lp), eight, 8);
}
int DistortionUpdate(oalgpu_effect *e, float rate, const void *props, const float*)
{   // DistortionState::update, distortion.cpp:141-195 (the filters work on the 4x oversampled signal)
    const auto &p = *static_cast<const oalgpu_distortion_props*>(props);
    const float edge = std::min(std::sin(kPiF * 0.5f * p.edge), 0.99f);
    e->G.edgeCoeff = 2.0f * edge / (1.0f - edge);
    float lp[5], bp[5];
    DesignBiquadFromBandwidth(OALGPU_BIQUAD_LOWPASS, p.lowpass_cutoff / rate * 0.25f, 1.0f, 0.746268656716f, lp);
    const float bandwidth = p.eq_bandwidth / (p.eq_center * 0.67f);
    DesignBiquadFromBandwidth(OALGPU_BIQUAD_BANDPASS, p.eq_center / rate * 0.25f, 1.0f, bandwidth, bp);
    for(uint32_t c = 0; c < 4; ++c)
    {
        if(int rc = UploadAt(e->st2.p, offsetof(Fx2State, lp) + c * sizeof(BiquadState) + offsetof(BiquadState, b0), lp, 5)) return rc;
        if(int rc = UploadAt(e->st2.p, offsetof(Fx2State, bp) + c * sizeof(BiquadState) + offsetof(BiquadState, b0), bp, 5)) return rc;
    }
    return OALGPU_OK;
}

int AutowahUpdate(oalgpu_effect *e, float rate, const void *props, const float*)
{   // AutowahState::update, autowah.cpp:100-122
    const auto &p = *static_cast<const oalgpu_autowah_props*>(props);
    Fx2Launch &G = e->G;
    const float release = std::min(std::max(p.release_time, 0.001f), 1.0f);
    G.attackRate = std::exp(-1.0f / (p.attack_time * rate));
    G.releaseRate = std::exp(-1.0f / (release * rate));
    G.resonanceGain = std::sqrt(std::log10(p.resonance) * 10.0f / 3.0f);
    G.peakGain = 1.0f - std::log10(p.peak_gain / 31621.0f);
    G.freqMinNorm = 20.0f / rate;
    G.bandwidthNorm = (2500.0f - 20.0f) / rate;
    return OALGPU_OK;
}

int VmorpherUpdate(oalgpu_effect *e, float rate, const void *props, const float*)
{   // VmorpherState::update, vmorpher.cpp:234-277; getFiltersByPhoneme :164-226
    const auto &p = *static_cast<const oalgpu_vmorpher_props*>(props);
    Fx2Launch &G = e->G;
    const float step = p.rate / rate;
    G.vmStep = RoundU(std::min(std::max(step * 16777216.0f, 0.0f), 16777216.0f - 1.0f));
    G.vmWave = G.vmStep == 0 ? 0 : p.waveform == OALGPU_VMORPHER_SINUSOID ? 1 : p.waveform == OALGPU_VMORPHER_TRIANGLE ? 2 : 3;
    static const float kFreq[5][4] = {{800, 1150, 2900, 3900}, {350, 2000, 2800, 3600}, {270, 2140, 2950, 3900},
        {450, 800, 2830, 3800}, {325, 700, 2700, 3800}};
    static const float kGain[5][4] = {{1.000000f, 0.501187f, 0.025118f, 0.100000f}, {1.000000f, 0.100000f, 0.177827f, 0.009999f},
        {1.000000f, 0.251188f, 0.050118f, 0.050118f}, {1.000000f, 0.281838f, 0.079432f, 0.079432f},
        {1.000000f, 0.158489f, 0.017782f, 0.009999f}};
    const int32_t ph[2] = {p.phoneme_a, p.phoneme_b}, tune[2] = {p.phoneme_a_coarse_tuning, p.phoneme_b_coarse_tuning};
    for(int v = 0; v < 2; ++v)
    {
        const float pitch = std::pow(2.0f, float(tune[v]) / 12.0f);
        for(int k = 0; k < 4; ++k)
        {
            if(ph[v] >= 0 && ph[v] < 5)
            {   // FormantFilter(f0norm, gain): mCoeff = tan(pi * f0norm)
                G.vmG[v * 4 + k] = std::tan(kPiF * ((kFreq[ph[v]][k] * pitch) / rate));
                G.vmGain[v * 4 + k] = kGain[ph[v]][k];
            }
            else { G.vmG[v * 4 + k] = 0.0f; G.vmGain[v * 4 + k] = 1.0f; }       // the other phonemes: FormantFilter{}
        }
    }
    // the copies of the new filters start with cleared histories, for every wet channel
    std::vector<float> zeros(size_t{e->numIn} * 16, 0.0f);
    return UploadAt(e->st2.p, offsetof(Fx2State, vmS), zeros.data(), zeros.size());
}
int VmorpherBegin(oalgpu_effect *e, uint32_t&) { e->G.vmIndex = e->vmorpher.index; return OALGPU_OK; }
void VmorpherAdvance(oalgpu_effect *e, uint32_t n)
{   // vmorpher.cpp:293-294
    for(uint32_t base = 0; base < n; base += 256u)
        e->vmorpher.index = (e->vmorpher.index + e->G.vmStep * std::min(256u, n - base)) & 0xffffffu;
}

int FshifterDeviceUpdate(oalgpu_effect *e, FxState&)
{   // FshifterState::deviceUpdate, fshifter.cpp:133-160; the Hann window of common/hann_window.hpp
    Fx2Launch &G = e->G; auto &fs = e->fshifter;
    HIP_TRY(fs.in.alloc_zero(4 * 1024));
    HIP_TRY(fs.outFifo.alloc_zero(4 * 256));
    HIP_TRY(fs.accum.alloc_zero(4 * 1024));
    HIP_TRY(fs.outdata.alloc_zero(4 * OALGPU_BUFFER_LINE_SIZE));
    std::vector<FsPair> tw; BuildTwiddles(tw);
    HIP_TRY(fs.tw.alloc(tw.size())); HIP_TRY(fs.tw.upload(tw.data(), tw.size()));
    // cos / sin of phase_idx * (pi*2 / MixerFracOne), fshifter.cpp:323-326: one entry per phase index
    std::vector<FsPair> ph(65536);
    for(uint32_t i = 0; i < 65536; ++i)
    {
        const double phase = i * (kPi * 2.0 / 65536.0);
        ph[i] = FsPair{std::cos(phase), std::sin(phase)};
    }
    HIP_TRY(fs.phase.alloc(ph.size())); HIP_TRY(fs.phase.upload(ph.data(), ph.size()));
    if(int rc = UploadHannWindow1024(fs.window)) return rc;
    G.fsIn = fs.in.p; G.fsOutFifo = fs.outFifo.p; G.fsAccum = fs.accum.p; G.fsOutdata = fs.outdata.p;
    G.fsTw = fs.tw.p; G.fsPhase = fs.phase.p; G.fsWindow = fs.window.p;
    for(int c = 0; c < 4; ++c) G.fsSign[c] = 1.0;
    return OALGPU_OK;
}
int FshifterUpdate(oalgpu_effect *e, float rate, const void *props, const float*)
{   // FshifterState::update, fshifter.cpp:162-214
    const auto &p = *static_cast<const oalgpu_fshifter_props*>(props);
    Fx2Launch &G = e->G;
    const float step = p.frequency / rate;
    const uint32_t phaseStep = RoundU(std::min(step, 1.0f) * 65536.0f);
    for(int c = 0; c < 4; ++c) G.fsPhaseStep[c] = phaseStep;
    const int32_t dir[2] = {p.left_direction, p.right_direction};
    for(int side = 0; side < 2; ++side)
        for(int c = side * 2; c < side * 2 + 2; ++c)
        {
            if(dir[side] == OALGPU_FSHIFTER_DOWN) G.fsSign[c] = -1.0;
            else if(dir[side] == OALGPU_FSHIFTER_UP) G.fsSign[c] = 1.0;
            else { e->fshifter.phase4[c] = 0; G.fsPhaseStep[c] = 0; }
        }
    return OALGPU_OK;
}
int FshifterBegin(oalgpu_effect *e, uint32_t&)
{
    e->G.fsCount = e->fshifter.hop.count; e->G.fsPos = e->fshifter.hop.pos;
    for(int c = 0; c < 4; ++c) e->G.fsPhaseIdx[c] = e->fshifter.phase4[c];
    return OALGPU_OK;
}
void FshifterAdvance(oalgpu_effect *e, uint32_t n)
{   // fshifter.cpp:228-259,330-336
    AdvanceHop(e->fshifter.hop, 256u, n);
    for(int c = 0; c < 4; ++c) e->fshifter.phase4[c] = (e->fshifter.phase4[c] + n * e->G.fsPhaseStep[c]) & 65535u;
}

int PshifterDeviceUpdate(oalgpu_effect *e, FxState&)
{   // PshifterState::deviceUpdate, pshifter.cpp:128-166: up to second order; pitch 1
    if(e->numIn > 9) return Fail(OALGPU_ERR_INVALID, "oalgpu_effect_create: the pitch shifter works on up to 9 channels (second order)");
    Fx2Launch &G = e->G; auto &ps = e->pshifter;
    HIP_TRY(ps.ring.alloc_zero(2 * 9 * 1024));
    HIP_TRY(ps.phase.alloc_zero(2 * 2 * 513));
    HIP_TRY(ps.accum.alloc_zero(9 * 1024));
    HIP_TRY(ps.outFifo.alloc_zero(9 * 128));
    HIP_TRY(ps.rows.alloc_zero(9 * OALGPU_BUFFER_LINE_SIZE));
    std::vector<float> tw(2 * 512);
    for(uint32_t m = 0; m < 512; ++m)
    {
        const double a = -2.0 * kPi * double(m) / 1024.0;
        tw[2 * m] = static_cast<float>(std::cos(a)); tw[2 * m + 1] = static_cast<float>(std::sin(a));
    }
    HIP_TRY(ps.tw.alloc(tw.size())); HIP_TRY(ps.tw.upload(tw.data(), tw.size()));
    if(int rc = UploadHannWindow1024(ps.window)) return rc;
    G.psAccum = ps.accum.p; G.psOutFifo = ps.outFifo.p; G.psRows = ps.rows.p;
    G.psTw = ps.tw.p; G.psWindow = ps.window.p;
    G.psPitchI = 65536u; G.psPitch = 1.0f;
    return OALGPU_OK;
}
int PshifterUpdate(oalgpu_effect *e, float, const void *props, const float*)
{   // PshifterState::update, pshifter.cpp:168-199
    const auto &p = *static_cast<const oalgpu_pshifter_props*>(props);
    const int32_t tune = p.coarse_tune * 100 + p.fine_tune;
    const float pitch = std::pow(2.0f, float(tune) / 1200.0f);
    e->G.psPitchI = RoundU(std::min(std::max(pitch, 0.5f), 2.0f) * 65536.0f);
    e->G.psPitch = float(e->G.psPitchI) * (1.0f / 65536.0f);
    return OALGPU_OK;
}
int PshifterBegin(oalgpu_effect *e, uint32_t&)
{
    Fx2Launch &G = e->G; auto &ps = e->pshifter;
    const uint32_t p = ps.parity;
    G.psRingIn = ps.ring.p + size_t{p} * 9 * 1024; G.psRingOut = ps.ring.p + size_t{p ^ 1u} * 9 * 1024;
    G.psPhaseIn = ps.phase.p + size_t{p} * 2 * 513; G.psPhaseOut = ps.phase.p + size_t{p ^ 1u} * 2 * 513;
    G.psCount = ps.hop.count; G.psPos = ps.hop.pos;
    return OALGPU_OK;
}
void PshifterAdvance(oalgpu_effect *e, uint32_t n) { e->pshifter.parity ^= 1u; AdvanceHop(e->pshifter.hop, 128u, n); }

// What the entry points need to know of a kind: one row per oalgpu_effect_kind, in its order.
struct KindInfo {
    const char *subject;                // how update's refusal names the kind
    bool fx2;                           // LaunchEffect2 (effects2_kernels.hip) instead of LaunchEffect (effects_kernels.hip)
    bool needProps, needTargets;        // what update may not be called without
    uint32_t upRows;                    // rows of the up-sampler set_upsampler installs: 4 A-Format, 9 second order, 0 none
    uint32_t maxWet;                    // the most wet channels it takes
    // allocation and defaults at create (`fresh`: the FxState an instance of the first five kinds starts from, uploaded afterwards)
    int (*deviceUpdate)(oalgpu_effect*, FxState &fresh);
    int (*update)(oalgpu_effect*, float rate, const void *props, const float *gains);   // props to launch constants
    int (*begin)(oalgpu_effect*, uint32_t &lds);        // the scalars process() reads, into the launch constants; the launch's dynamic LDS
    void (*advance)(oalgpu_effect*, uint32_t n);        // what process() does to those scalars
};
constexpr KindInfo kKinds[OALGPU_EFFECT_PSHIFTER + 1] = {
    {"equalizer",   false, true,  true,  0, kFxMaxIn, nullptr, EqualizerUpdate, nullptr, nullptr},
    {"modulator",   false, true,  true,  0, kFxMaxIn, nullptr, ModulatorUpdate, ModulatorBegin, ModulatorAdvance},
    {"echo",        false, true,  false, 0, kFxMaxIn, EchoDeviceUpdate, EchoUpdate, EchoBegin, EchoAdvance},
    {"dedicated",   false, false, false, 0, kFxMaxIn, nullptr, DedicatedUpdate, nullptr, nullptr},
    {"compressor",  false, true,  true,  0, kFxMaxIn, CompressorDeviceUpdate, CompressorUpdate, nullptr, nullptr},
    {"this effect", true,  true,  true,  4, 4,        ChorusDeviceUpdate, ChorusUpdate, ChorusBegin, ChorusAdvance},
    {"this effect", true,  true,  true,  4, 4,        DistortionDeviceUpdate, DistortionUpdate, nullptr, nullptr},
    {"this effect", true,  true,  true,  0, kFxMaxIn, nullptr, AutowahUpdate, nullptr, nullptr},
    {"this effect", true,  true,  true,  0, kFxMaxIn, nullptr, VmorpherUpdate, VmorpherBegin, VmorpherAdvance},
    {"this effect", true,  true,  true,  4, 4,        FshifterDeviceUpdate, FshifterUpdate, FshifterBegin, FshifterAdvance},
    {"this effect", true,  true,  true,  9, 9,        PshifterDeviceUpdate, PshifterUpdate, PshifterBegin, PshifterAdvance},
};

// mChans[c].mTargetChannel / mTargetGain of the first `chans` wet channels (no `gains`: the up-sampler's rows hold them)
template<typename Launch>
void SetTargets(Launch &L, uint32_t chans, const uint32_t *target_channels, const float *gains)
{
    for(uint32_t ch = 0; ch < kFxMaxIn; ++ch) { L.target[ch] = OALGPU_INVALID_CHANNEL; L.tgtGain[ch] = 0.0f; }
    for(uint32_t ch = 0; ch < chans; ++ch) { L.target[ch] = target_channels[ch]; if(gains) L.tgtGain[ch] = gains[ch]; }
}

} // namespace

extern "C" {

int oalgpu_effect_create(int device, int math_mode, int kind, uint32_t sample_rate, uint32_t num_in_channels,
    uint32_t num_out_lines, oalgpu_effect **out)
{
    if(!out || kind < OALGPU_EFFECT_EQUALIZER || kind > OALGPU_EFFECT_PSHIFTER || sample_rate < 8000 || num_in_channels < 1
        || num_in_channels > kFxMaxIn || num_out_lines < 1 || num_out_lines > OALGPU_MAX_OUTPUT_CHANNELS)
        return Fail(OALGPU_ERR_INVALID, "oalgpu_effect_create: bad arguments");
    *out = nullptr;
    if(int rc = UseDevice(device)) return rc;
    const KindInfo &K = kKinds[kind];
    auto e = std::make_unique<oalgpu_effect>();
    e->device = device; e->kind = kind; e->sampleRate = sample_rate; e->numIn = num_in_channels; e->nlines = num_out_lines;
    HIP_TRY(e->st.alloc_zero(1));
    HIP_TRY(e->tgtGains.alloc_zero(2 * OALGPU_MAX_OUTPUT_CHANNELS));
    HIP_TRY(e->hostIn.alloc(size_t{num_in_channels} * OALGPU_BUFFER_LINE_SIZE));
    HIP_TRY(e->hostOut.alloc(size_t{num_out_lines} * OALGPU_BUFFER_LINE_SIZE));
    FxLaunch &F = e->F;
    F.kind = kind; F.exact = math_mode == OALGPU_MATH_EXACT ? 1 : 0; F.numIn = num_in_channels; F.nlines = num_out_lines;
    F.st = e->st.p; F.tgtGains = e->tgtGains.p;
    SetTargets(F, 0, nullptr, nullptr);
    F.modRange = 1; F.modWave = 0;
    if(K.fx2)
    {
        HIP_TRY(e->st2.alloc_zero(1));
        HIP_TRY(e->upTgt.alloc_zero(9 * 32));
        Fx2Launch &G = e->G;
        G.kind = kind; G.numIn = num_in_channels; G.nlines = num_out_lines; G.st = e->st2.p; G.upTgt = e->upTgt.p;
        SetTargets(G, 0, nullptr, nullptr);
        G.hfScale[0] = G.hfScale[1] = 1.0f; G.lfoRange = 1;
    }
    FxState fresh{};                     // a BiquadFilter starts as the identity (mB0 = 1)
    for(auto &chan : fresh.bq) for(BiquadState &b : chan) b.b0 = 1.0f;
    if(K.deviceUpdate) { if(int rc = K.deviceUpdate(e.get(), fresh)) return rc; }
    if(!K.fx2) HIP_TRY(e->st.upload(&fresh, 1));
    *out = e.release();
    return OALGPU_OK;
}

void oalgpu_effect_destroy(oalgpu_effect *e)
{
    if(!e) return;
    (void)UseDevice(e->device);          // (a resident voice kernel on the device is told to leave first: it would sit out the synchronisation until its watchdog)
    (void)hipDeviceSynchronize();
    delete e;
}

int oalgpu_effect_update(oalgpu_effect *e, const void *props, const uint32_t *target_channels, const float *gains)
{
    if(!e || !gains) return Fail(OALGPU_ERR_INVALID, "oalgpu_effect_update: null argument");
    if(int rc = UseDevice(e->device)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    const KindInfo &K = kKinds[e->kind];
    if((K.needProps && !props) || (K.needTargets && !target_channels))
        return Fail(OALGPU_ERR_INVALID, std::string("oalgpu_effect_update: ") + K.subject + " needs props" + (K.needTargets ? " and targets" : ""));
    if(int rc = K.update(e, float(e->sampleRate), props, gains)) return rc;
    if(K.needTargets)
    {
        const bool up = K.upRows && e->G.upsample;
        if(up)
        {   // UpsampleParams::mTargetGains = ComputePanGains(target.Main, AmbiScale::FirstOrderUp[ch] (pitch shifter: SecondOrderUp[ch]),
            // gain): gains[4 or 9][num_out_lines]
            std::vector<float> rows(9 * 32, 0.0f);
            for(uint32_t ch = 0; ch < K.upRows; ++ch)
                for(uint32_t l = 0; l < e->nlines; ++l) rows[ch * 32 + l] = gains[size_t{ch} * e->nlines + l];
            HIP_TRY(e->upTgt.upload(rows.data(), rows.size()));
        }
        const uint32_t chans = std::min(e->numIn, K.maxWet);
        if(K.fx2) SetTargets(e->G, chans, target_channels, up ? nullptr : gains);
        else SetTargets(e->F, chans, target_channels, gains);
    }
    e->updated = true;
    return OALGPU_OK;
}

/* deviceUpdate on a device above first order (chorus.cpp:143-162 and alike): mUpsampler */
int oalgpu_effect_set_upsampler(oalgpu_effect *e, const float order_scales[2], float xover_norm)
{
    if(!e) return Fail(OALGPU_ERR_INVALID, "null argument");
    if(!kKinds[e->kind].upRows)
        return Fail(OALGPU_ERR_INVALID, "oalgpu_effect_set_upsampler: only the chorus, the distortion and the frequency / pitch shifters up-sample");
    if(e->nlines > 32) return Fail(OALGPU_ERR_INVALID, "oalgpu_effect_set_upsampler: at most 32 output lines");
    if(int rc = UseDevice(e->device)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    Fx2Launch &G = e->G;
    G.upsample = order_scales ? 1 : 0;
    if(order_scales)
    {
        G.hfScale[0] = order_scales[0]; G.hfScale[1] = order_scales[1];
        G.splitCoeff = SplitterCoeff(xover_norm);
    }
    // a fresh BandSplitter and zeroed gains, as deviceUpdate leaves them
    std::vector<float> zeros(9 * 32 + 9 * 3, 0.0f);
    if(int rc = UploadAt(e->st2.p, offsetof(Fx2State, upCur), zeros.data(), zeros.size())) return rc;
    e->updated = false;
    return OALGPU_OK;
}

} // extern "C"

int oalgpu_effect_process_device(oalgpu_effect *e, void *hip_stream, const float *wet_in_dev, float *out_lines_dev, uint32_t n)
{
    if(!e || !wet_in_dev || !out_lines_dev || n == 0 || n > OALGPU_BUFFER_LINE_SIZE)
        return Fail(OALGPU_ERR_INVALID, "oalgpu_effect_process: bad arguments");
    if(!e->updated) return Fail(OALGPU_ERR_INVALID, "oalgpu_effect_process: no update() yet");
    if(int rc = UseDevice(e->device)) return rc;
    const KindInfo &K = kKinds[e->kind];
    uint32_t lds = 0;
    if(K.begin) { if(int rc = K.begin(e, lds)) return rc; }
    const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if(K.fx2) { Fx2Launch G = e->G; G.wetIn = wet_in_dev; G.outLines = out_lines_dev; G.n = n; LaunchEffect2(stream, G, lds); }
    else { FxLaunch F = e->F; F.wetIn = wet_in_dev; F.outLines = out_lines_dev; F.n = n; LaunchEffect(stream, F); }
    HIP_TRY(hipGetLastError());
    if(K.advance) K.advance(e, n);
    return OALGPU_OK;
}

extern "C" int oalgpu_effect_process(oalgpu_effect *e, const float *wet_in, float *out_lines, uint32_t n)
{
    if(!e || !wet_in || !out_lines) return Fail(OALGPU_ERR_INVALID, "null argument");
    if(int rc = UseDevice(e->device)) return rc;
    const size_t inFloats = size_t{e->numIn} * OALGPU_BUFFER_LINE_SIZE, outFloats = size_t{e->nlines} * OALGPU_BUFFER_LINE_SIZE;
    HIP_TRY(hipMemcpy(e->hostIn.p, wet_in, inFloats * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->hostOut.p, out_lines, outFloats * sizeof(float), hipMemcpyHostToDevice));
    if(int rc = oalgpu_effect_process_device(e, nullptr, e->hostIn.p, e->hostOut.p, n)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out_lines, e->hostOut.p, outFloats * sizeof(float), hipMemcpyDeviceToHost));
    return OALGPU_OK;
}

namespace oalgpu {
uint32_t EffectOutLines(const oalgpu_effect *e) { return e ? e->nlines : 0u; }
uint32_t EffectInChannels(const oalgpu_effect *e) { return e ? e->numIn : 0u; }
}
