#include "params.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "tables.hpp"

namespace oalgpu {
namespace {

constexpr uint32_t kFracOne = 1u << OALGPU_MIXER_FRAC_BITS;

int BsincFamily(int resampler)
{
    switch(resampler)
    {
    case OALGPU_RESAMPLER_FAST_BSINC12: case OALGPU_RESAMPLER_BSINC12: return 12;
    case OALGPU_RESAMPLER_FAST_BSINC24: case OALGPU_RESAMPLER_BSINC24: return 24;
    default: return 48;
    }
}

} // namespace

void PrepareResampler(int resampler, uint32_t increment, oalgpu_interp_state *out)
{
    *out = oalgpu_interp_state{};
    switch(resampler)
    {
    case OALGPU_RESAMPLER_POINT: out->kind = 0; return;
    case OALGPU_RESAMPLER_LINEAR: out->kind = 1; return;
    case OALGPU_RESAMPLER_SPLINE: out->kind = 2; out->table = 0; return;
    case OALGPU_RESAMPLER_GAUSSIAN: out->kind = 2; out->table = 1; return;
    default: break;
    }
    const bool fastOnly = resampler == OALGPU_RESAMPLER_FAST_BSINC12
        || resampler == OALGPU_RESAMPLER_FAST_BSINC24 || resampler == OALGPU_RESAMPLER_FAST_BSINC48;
    const int family = BsincFamily(resampler);
    const BsincTable *table = GetBsincTable(family);

    // BsincPrepare: scale index + curve-fitted interpolation factor when down-sampling.
    uint32_t si = 15;
    float sf = 0.0f;
    if(increment > kFracOne) BsincScale(table->scaleBase, table->scaleRange, increment, si, sf);
    out->kind = (!fastOnly && increment > kFracOne) ? 4 : 3;
    out->table = family;
    out->sf = sf;
    out->m = table->m[si];
    out->l = out->m / 2u - 1u;
    out->filter_offset = table->filterOffset[si];
}

void DesignBiquadFromBandwidth(int type, float f0norm, float gain, float bandwidth, float c[5])
{   // rcpQFromBandwidth, biquad.h:71-75
    const float w0 = 3.14159265358979323846f * 2.0f * f0norm;
    DesignBiquad(type, f0norm, gain, 2.0f * std::sinh(std::log(2.0f) / 2.0f * bandwidth * w0 / std::sin(w0)), c);
}

void ApplyBiquadTarget(oalgpu_biquad *f, const float c[5])
{
    float *tgt[5] = {&f->tb0, &f->tb1, &f->tb2, &f->ta1, &f->ta2};
    bool changed = false;
    for(int i = 0; i < 5; ++i)
    {
        changed |= !(std::fabs(c[i] - *tgt[i]) <= 0.015625f);
        *tgt[i] = c[i];
    }
    auto snap = [f] {
        f->counter = 0;
        f->b0 = f->tb0; f->b1 = f->tb1; f->b2 = f->tb2; f->a1 = f->ta1; f->a2 = f->ta2;
    };
    if(!changed) { if(f->counter <= 0) snap(); }
    else if(f->counter >= 0) f->counter = 8 * 32;   // InterpSteps * SamplesPerStep
    else snap();
}

float SplitterCoeff(float f0norm)
{
    const float w = 3.14159265358979323846f * 2.0f * std::min(f0norm, 0.49f);
    const float cw = std::cos(w);
    if(cw > 1.1920928955078125e-07f) return (std::sin(w) - 1.0f) / cw;
    return cw * -0.5f;
}

// (the sections' arithmetic: csrc/dev_nfc_design.hpp, shared with SourceNfcKernel)
void NfcInit(float w1, NfcDesign &d)
{
    std::memset(&d, 0, sizeof(d));
    for(int o = 1; o <= 4; ++o)
    {
        const float g = NfcOrderDesign(uint32_t(o), w1, d.a[o]);
        d.baseGain[o] = 1.0f / g;
        d.a[o][0] = 1.0f;
        for(int k = 1; k <= o; ++k) d.b[o][k] = d.a[o][k];
    }
}

void NfcAdjust(float w0, NfcDesign &d)
{
    for(int o = 1; o <= 4; ++o)
    {
        const float g = NfcOrderDesign(uint32_t(o), w0, d.b[o]);
        d.a[o][0] = d.baseGain[o] * g;
    }
}

} // namespace oalgpu
