// The stereo UHJ encoder: UhjPostProcess (alc/alu.cpp:300-311) over the dry lines W, X, Y and the two real output lines,
// one workgroup of four wavefronts per context and update.  The IIR and FIR-N forms are those of dev_encoder.hpp with
// UhjEncoderIIR's / UhjEncoder<N>'s input mixes (core/uhjfilter.cpp) and Y's gain 0.267586995182 in D.
#include "dev_encoder.hpp"

#pragma clang fp contract(off)

namespace oalgpu {
namespace {

constexpr uint32_t kUhjThreads = kEncThreads;
constexpr float kUhjYGain = 0.267586995182f;

// S = 0.4698463 W + 0.0757602682546 X; the W/X part of D = j(-0.17101005 W + 0.208149636675 X)
struct UhjMix {
    const float *w, *x, *y;
    __device__ __forceinline__ void operator()(uint32_t i, float &s, float &wx, float &yv) const
    {
        const float wv = w[i], xv = x[i];
        s = 0.4698463f * wv + 0.0757602682546f * xv;
        wx = -0.17101005f * wv + 0.208149636675f * xv;
        yv = y[i];
    }
};

__global__ __launch_bounds__(kUhjThreads) void UhjIirKernel(float *left, float *right, const float *w, const float *x,
    const float *y, uint32_t n, float *state)
{
    EncodeIir(left, right, n, state, kUhjYGain, UhjMix{w, x, y});
}

template<uint32_t N>
__global__ __launch_bounds__(kUhjThreads) void UhjFirKernel(float *left, float *right, const float *w, const float *x,
    const float *y, uint32_t n, const float *taps, float *state)
{
    EncodeFir<N>(left, right, n, taps, state, kUhjYGain, UhjMix{w, x, y});
}

} // namespace

void LaunchUhjEncode(hipStream_t s, int quality, float *left, float *right, const float *w, const float *x, const float *y,
    uint32_t n, const float *taps, float *state)
{
    if(quality == kUhjIir)
        hipLaunchKernelGGL(UhjIirKernel, dim3(1), dim3(kUhjThreads), 0, s, left, right, w, x, y, n, state);
    else if(quality == kUhjFir256)
        hipLaunchKernelGGL(UhjFirKernel<256>, dim3(1), dim3(kUhjThreads), 0, s, left, right, w, x, y, n, taps, state);
    else
        hipLaunchKernelGGL(UhjFirKernel<512>, dim3(1), dim3(kUhjThreads), 0, s, left, right, w, x, y, n, taps, state);
}

size_t UhjStateFloats(int quality)
{
    if(quality == kUhjIir) return kEncIirStateFloats;
    return EncFirStateFloats(UhjFirLength(quality));
}

} // namespace oalgpu
