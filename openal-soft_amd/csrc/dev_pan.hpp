// CalcDirectionCoeffs / CalcAmbiCoeffs (core/mixer.h:68-73, core/ambidefs.h:219-271, core/mixer.cpp:16-90) and one line of
// ComputePanGains (core/mixer.cpp:92-102), for the device (PanGainsKernel, SourceParamsKernel) and for the host
// (oalgpu_source_params_host): the ONE coefficient an AmbiMap entry names, in the reference's operation order (no
// contraction), so that a direction without spread yields bit-identical gains.  The spread's zonal scaling uses cos and
// sqrt: within an ulp or two of the host's libm on the device.
#pragma once
#include "dev_design.hpp"

#pragma clang fp contract(off)

namespace oalgpu {

// ACN `acn` of CalcAmbiCoeffs(y, z, x) (ambisonic coordinates), core/ambidefs.h:219-271
OALGPU_HD inline float AmbiCoeff(uint32_t acn, float y, float z, float x)
{
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    switch(acn)
    {
    case 0: return 1.0f;
    case 1: return 1.7320508075688772f * y;
    case 2: return 1.7320508075688772f * z;
    case 3: return 1.7320508075688772f * x;
    case 4: return 3.872983346e+00f * xy;
    case 5: return 3.872983346e+00f * yz;
    case 6: return 1.118033989e+00f * (3.0f * zz - 1.0f);
    case 7: return 3.872983346e+00f * xz;
    case 8: return 1.936491673e+00f * (xx - yy);
    case 9: return 2.091650066e+00f * (y * (3.0f * xx - yy));
    case 10: return 1.024695076e+01f * (z * xy);
    case 11: return 1.620185175e+00f * (y * (5.0f * zz - 1.0f));
    case 12: return 1.322875656e+00f * (z * (5.0f * zz - 3.0f));
    case 13: return 1.620185175e+00f * (x * (5.0f * zz - 1.0f));
    case 14: return 5.123475383e+00f * (z * (xx - yy));
    case 15: return 2.091650066e+00f * (x * (xx - 3.0f * yy));
    case 16: return 8.874119675e+00f * (xy * (xx - yy));
    case 17: return 6.274950199e+00f * ((3.0f * xx - yy) * yz);
    case 18: return 3.354101966e+00f * (xy * (7.0f * zz - 1.0f));
    case 19: return 2.371708245e+00f * (yz * (7.0f * zz - 3.0f));
    case 20: return 3.750000000e-01f * (35.0f * (zz * zz) - 30.0f * zz + 3.0f);
    case 21: return 2.371708245e+00f * (xz * (7.0f * zz - 3.0f));
    case 22: return 1.677050983e+00f * ((xx - yy) * (7.0f * zz - 1.0f));
    case 23: return 6.274950199e+00f * ((xx - 3.0f * yy) * xz);
    default: return 2.218529919e+00f * ((xx * xx) - 6.0f * (xx * yy) + (yy * yy));
    }
}

// the spread's zonal-harmonic factor of ambisonic order `order`, core/mixer.cpp:20-86
OALGPU_HD inline float SpreadFactor(uint32_t order, float spread)
{
    const float ca = cosf(spread * 0.5f);
    const float scale = sqrtf(1.0f + 0.31830988618379067154f * 0.5f * spread);
    const float caca = ca * ca;
    switch(order)
    {
    case 0: return scale;
    case 1: return scale * 0.5f * (ca + 1.0f);
    case 2: return scale * 0.5f * ((ca + 1.0f) * ca);
    case 3: return scale * 0.125f * ((ca + 1.0f) * (5.0f * caca - 1.0f));
    default: return scale * 0.125f * ((ca + 1.0f) * (7.0f * caca - 3.0f) * ca);
    }
}

// gains[line] of ComputePanGains (core/mixer.cpp:99) for the line whose AmbiMap entry is {index, scale}: the coefficient of
// CalcDirectionCoeffs(dir, spread) -- (y, z, x) = (-dir[0], dir[1], -dir[2]), core/mixer.h:71-72 -- times the scale and the gain
OALGPU_HD inline float PanLineGain(uint32_t index, float scale, float y, float z, float x, float spread, float ingain)
{
    float c = AmbiCoeff(index, y, z, x);
    if(spread > 0.0f)
    {
        const uint32_t order = index == 0 ? 0u : (index < 4 ? 1u : (index < 9 ? 2u : (index < 16 ? 3u : 4u)));
        c *= SpreadFactor(order, spread);
    }
    return scale * c * ingain;
}

} // namespace oalgpu
