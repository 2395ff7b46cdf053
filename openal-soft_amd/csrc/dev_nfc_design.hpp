// NfcFilter's coefficient design (core/filters/nfc.cpp:49-203), once, for the host (host/params.cpp: NfcInit, NfcAdjust; plain
// C++) and for the device (SourceNfcKernel, source_nfc_kernels.hip).  A filter of order 1..4 is a cascade of at most two
// sections, second order first: order 1 = {first}, 2 = {second}, 3 = {second, first}, 4 = {second, second}.  Only + * / in the
// reference's operation order, no contraction: host and device agree bit for bit.
#pragma once
#include "dev_design.hpp"

#pragma clang fp contract(off)

namespace oalgpu {

constexpr uint32_t kNfcSections = 6;

// the Bessel constants of section s (B1 .. B4, nfc.cpp:49-52) as (k1, k2): b_0 = k1 * r, b_1 = k2 * r * r.  The six sections
// in the order they are numbered here -- 0: order 1; 1: order 2; 2, 3: order 3 (second, first); 4, 5: order 4 -- selected by
// comparisons (a table would be indexed per lane on the device)
OALGPU_HD inline void NfcSectionConsts(uint32_t s, float &k1, float &k2)
{
    k1 = s == 0u ? 1.0f : (s == 1u ? 3.0f : (s == 2u ? 3.6778f : (s == 3u ? 2.3222f : (s == 4u ? 4.2076f : 5.7924f))));
    k2 = s == 0u ? 0.0f : (s == 1u ? 3.0f : (s == 2u ? 6.4595f : (s == 3u ? 0.0f : (s == 4u ? 11.4877f : 9.1401f))));
}

// One section at r = w / 2: its gain factor g = 1 + b_0 + b_1 and its two coefficients (2 b_0 + 4 b_1) / g and 4 b_1 / g
// (NfcFilterCreate2 / NfcFilterAdjust2, nfc.cpp:76-103, :160-172).  A first-order section (NfcFilterCreate1, :56-74: g = 1 + b_0,
// 2 b_0 / g) is the same with k2 = 0: b_1 is +0 then, and x + (+0) = x for the x >= 0 of this design, so the sums keep their bits.
OALGPU_HD inline float NfcSectionDesign(uint32_t s, float r, float &c1, float &c2)
{
    float k1, k2;
    NfcSectionConsts(s, k1, k2);
    const float b0 = k1 * r, b1 = k2 * (r * r);
    const float g = 1.0f + b0 + b1;
    c1 = (2.0f * b0 + 4.0f * b1) / g;
    c2 = 4.0f * b1 / g;
    return g;
}

// the first section of the filter of order o (1..4); an order above 2 has the next one too
OALGPU_HD inline uint32_t NfcFirstSection(uint32_t o) { return o == 1u ? 0u : (o == 2u ? 1u : (o == 3u ? 2u : 4u)); }

// the filter of order o at angular frequency w: the coefficients into out[1..o], the product of the sections' gain factors back
OALGPU_HD inline float NfcOrderDesign(uint32_t o, float w, float *out)
{
    const float r = 0.5f * w;
    const uint32_t first = NfcFirstSection(o);
    float c1, c2;
    const float g1 = NfcSectionDesign(first, r, c1, c2);
    out[1] = c1;
    if(o == 1u) return g1;
    out[2] = c2;
    if(o == 2u) return g1;
    const float g0 = NfcSectionDesign(first + 1u, r, c1, c2);
    out[3] = c1;
    if(o == 4u) out[4] = c2;
    return g1 * g0;
}

} // namespace oalgpu
