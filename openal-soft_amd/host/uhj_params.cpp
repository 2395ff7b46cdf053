// SegmentedFilter<N>'s time-domain response (core/allpass_conv.hpp) restated: the reference builds it in double,
// splits it into 128-sample segments and convolves by FFT; the encoder's output is the same linear FIR, so the GPU
// applies the response directly.  Only the odd taps are nonzero.
#include "uhj_params.hpp"

#include <cmath>

namespace oalgpu {

uint32_t UhjFirLength(int quality)
{
    return quality == kUhjFir256 ? 256u : quality == kUhjFir512 ? 512u : 0u;
}

uint32_t UhjEncoderDelay(int quality)
{
    if(quality == kUhjIir) return 1u;
    const uint32_t n = UhjFirLength(quality);
    return n ? n / 2u + 128u : 0u;          // sFilterDelay = N/2 + sSegmentSize
}

std::vector<float> UhjFirTaps(uint32_t n)
{
    const double pi = 3.14159265358979323846;
    const uint32_t half = n / 2u;
    std::vector<float> taps(half);
    for(uint32_t i = 0; i < half; ++i)
    {
        const int k = int(half) - int(i * 2u + 1u);
        // the Blackman-Nuttall window over FilterHalfSize - 1
        const double w = 2.0 * pi / double(half - 1u) * double(i);
        const double window = 0.3635819 - 0.4891775 * std::cos(w) + 0.1365995 * std::cos(2.0 * w) - 0.0106411 * std::cos(3.0 * w);
        const double pk = pi * double(k);
        taps[i] = float(window * 2.0 / pk);
    }
    return taps;
}

} // namespace oalgpu
