// The stereo TSME encoder ("tetraphonic surround matrix encoding"): TsmePostProcess (alc/alu.cpp:314-327) over the dry lines
// W, Y, Z, X (ACN order, N3D scale) and the two real output lines, one workgroup of four wavefronts per context and update.
// The IIR and FIR-N forms are those of dev_encoder.hpp with TsmeEncoderIIR's / TsmeEncoder<N>'s input mixes
// (core/tsmefilter.cpp:137-329) and Y's gain 0.333238912931 in D.
//
// S = (0.288397341271 W + 0.166565447888 X) + 0.187684284734 Z is two statements in the reference, the W/X sum rounded before
// Z joins it.  FIR-N computes S from the delayed W, X, Z sample by sample; the delayed S of the undelayed lines is the same
// arithmetic on the same values, so S is mixed first and delayed as one line, as in the UHJ encoder.  The W/X part of D is
// written with a subtraction in the IIR form and with a negative constant in the FIR form, as the reference writes them.
#include "dev_encoder.hpp"

#pragma clang fp contract(off)

namespace oalgpu {
namespace {

constexpr uint32_t kTsmeThreads = kEncThreads;
constexpr float kTsmeYGain = 0.333238912931f;

template<bool Iir>
struct TsmeMix {
    const float *w, *y, *z, *x;
    __device__ __forceinline__ void operator()(uint32_t i, float &s, float &wx, float &yv) const
    {
        const float wv = w[i], xv = x[i];
        const float sum = 0.288397341271f * wv + 0.166565447888f * xv;
        s = sum + 0.187684284734f * z[i];
        wx = Iir ? 0.444008050325f * wv - 0.256439256487f * xv : 0.444008050325f * wv + -0.256439256487f * xv;
        yv = y[i];
    }
};

__global__ __launch_bounds__(kTsmeThreads) void TsmeIirKernel(float *left, float *right, const float *w, const float *y,
    const float *z, const float *x, uint32_t n, float *state)
{
    EncodeIir(left, right, n, state, kTsmeYGain, TsmeMix<true>{w, y, z, x});
}

template<uint32_t N>
__global__ __launch_bounds__(kTsmeThreads) void TsmeFirKernel(float *left, float *right, const float *w, const float *y,
    const float *z, const float *x, uint32_t n, const float *taps, float *state)
{
    EncodeFir<N>(left, right, n, taps, state, kTsmeYGain, TsmeMix<false>{w, y, z, x});
}

} // namespace

void LaunchTsmeEncode(hipStream_t s, int quality, float *left, float *right, const float *dry, uint32_t n, const float *taps,
    float *state)
{
    const float *w = dry, *y = dry + kLine, *z = dry + 2 * kLine, *x = dry + 3 * kLine;
    if(quality == kUhjIir)
        hipLaunchKernelGGL(TsmeIirKernel, dim3(1), dim3(kTsmeThreads), 0, s, left, right, w, y, z, x, n, state);
    else if(quality == kUhjFir256)
        hipLaunchKernelGGL(TsmeFirKernel<256>, dim3(1), dim3(kTsmeThreads), 0, s, left, right, w, y, z, x, n, taps, state);
    else
        hipLaunchKernelGGL(TsmeFirKernel<512>, dim3(1), dim3(kTsmeThreads), 0, s, left, right, w, y, z, x, n, taps, state);
}

} // namespace oalgpu
