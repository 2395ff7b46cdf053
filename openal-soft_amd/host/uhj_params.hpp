// Host-side constants of the UHJ encoder (core/uhjfilter.h, core/allpass_conv.hpp): its delays and the FIR
// qualities' phase-shift taps.  See uhj_params.cpp.
#pragma once
#include <stdint.h>

#include <vector>

namespace oalgpu {

enum : int { kUhjIir = 0, kUhjFir256 = 1, kUhjFir512 = 2 };   // UhjQualityType order

// UhjEncoder*::getDelay: 1 (IIR), N/2 + 128 (FIR-N); 0 for a quality that is not one of the three
uint32_t UhjEncoderDelay(int quality);
// FIR-N's filter length N (256 or 512); 0 for IIR or an invalid quality
uint32_t UhjFirLength(int quality);
// The N/2 nonzero taps of SegmentedFilter<N>'s response, h[2i+1] for i = 0 .. N/2-1, computed in double and
// rounded to float once
std::vector<float> UhjFirTaps(uint32_t n);

} // namespace oalgpu
