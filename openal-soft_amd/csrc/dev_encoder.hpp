// What the stereo matrix encoders share (uhj_kernels.hip: UhjEncoderIIR / UhjEncoder<N>, core/uhjfilter.cpp; tsme_kernels.hip:
// TsmeEncoderIIR / TsmeEncoder<N>, core/tsmefilter.cpp).  The two differ in how the dry lines mix into S, the W/X part of D
// and Y, and in Y's gain in D; everything behind the mix is the same code in the reference and the same code here.
//
// IIR.  Each all-pass section of allpass_iir.hpp computes y_n = c x_n + z0 with z0 = c y_{n-2} - x_{n-2}: even and odd
// samples form independent chains through all four sections.  The five cascades (S, the W/X mix of D, Y, the two direct
// lines) x two parities are ten serial chains, one lane each on wavefront 0, their inputs and outputs staged in LDS; the input
// mixes, the one-sample delays and the final combine run 256 samples wide.  The reference's float operations in its order
// (mul then add, (S + D) + direct): bit-identical.
//
// FIR-N.  The reference's segmented FFT convolution is the linear FIR jwx[t] = sum_i h[2i+1] wx[t - 128 - (2i+1)]
// (host/uhj_params.cpp); here a direct sum over the N/2 nonzero taps, one sample per thread, accumulated in double.  S, Y
// and the direct lines are delayed by N/2 + 128.  Histories live in the context's state buffer and are staged in LDS with the
// update's samples behind them.
//
// mix(i, s, wx, y): sample i of the three cascade inputs, in the reference's operations.
#pragma once
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace oalgpu {

constexpr uint32_t kEncThreads = 256;
constexpr float kEncF1[4] = {0.479400865589f, 0.876218493539f, 0.976597589508f, 0.997499255936f};   // Filter1Coeff
constexpr float kEncF2[4] = {0.161758498368f, 0.733028932341f, 0.945349700329f, 0.990599156684f};   // Filter2Coeff
constexpr size_t kEncIirStateFloats = 44;

// state (kEncIirStateFloats): [cascade][section][z0, z1] for the cascades S, WX, Y, L, R (40 floats) | the carried samples of
// S, Y, left, right (the encoders' mDelay* and mDirectDelay)
template<typename Mix>
__device__ __forceinline__ void EncodeIir(float *left, float *right, uint32_t n, float *state, float yGain, Mix &&mix)
{
    __shared__ float buf[5][kLine];            // the cascades' inputs, overwritten by their outputs
    const uint32_t t = threadIdx.x;
    for(uint32_t i = t; i < n; i += kEncThreads)
    {
        mix(i, buf[0][i], buf[1][i], buf[2][i]);
        buf[3][i] = left[i];
        buf[4][i] = right[i];
    }
    __syncthreads();
    if(t < 10u)
    {
        const uint32_t casc = t >> 1, par = t & 1u;
        float c[4], s[4];
#pragma unroll
        for(int k = 0; k < 4; ++k)
        {
            c[k] = casc == 1u ? kEncF2[k] : kEncF1[k];
            s[k] = state[casc * 8u + uint32_t(k) * 2u + par];
        }
        float *line = buf[casc];
#pragma unroll 4
        for(uint32_t i = par; i < n; i += 2u)
        {
            float v = line[i];
#pragma unroll
            for(int k = 0; k < 4; ++k)
            {
                const float yk = v * c[k] + s[k];
                s[k] = yk * c[k] - v;
                v = yk;
            }
            line[i] = v;
        }
        // z0 takes the chain of the update's second-to-last sample, z1 the last's (for n = 1 the odd chain's
        // value moves to z0 untouched)
        const uint32_t slot = (n & 1u) ? (par ^ 1u) : par;
#pragma unroll
        for(int k = 0; k < 4; ++k) state[casc * 8u + uint32_t(k) * 2u + slot] = s[k];
    }
    __syncthreads();
    float *carry = state + 40;
    for(uint32_t i = t; i < n; i += kEncThreads)
    {
        // S and Y, and the direct lines, through the one-sample delay
        const float sv = i ? buf[0][i - 1] : carry[0];
        const float yv = i ? buf[2][i - 1] : carry[1];
        const float lv = i ? buf[3][i - 1] : carry[2];
        const float rv = i ? buf[4][i - 1] : carry[3];
        const float dv = buf[1][i] + yGain * yv;
        left[i] = sv + dv + lv;
        right[i] = sv - dv + rv;
    }
    __syncthreads();                           // (thread 0 read the old carried samples above)
    if(t == 0)
    {
        carry[0] = buf[0][n - 1]; carry[1] = buf[2][n - 1];
        carry[2] = buf[3][n - 1]; carry[3] = buf[4][n - 1];
    }
}

// state (EncFirStateFloats(N)): the W/X mix's history (N + 127) | the last d samples of S, Y, left, right (d = N/2 + 128).
// LDS: (N + 127 + 1024) + 4 (N/2 + 128 + 1024) floats = 29180 bytes for N = 512.
template<uint32_t N, typename Mix>
__device__ __forceinline__ void EncodeFir(float *left, float *right, uint32_t n, const float *taps, float *state, float yGain,
    Mix &&mix)
{
    constexpr uint32_t kH = N + 127u, kD = N / 2u + 128u;
    __shared__ float wx[kH + kLine];
    __shared__ float dl[4][kD + kLine];        // [history | this update's] of S, Y, left, right
    const uint32_t t = threadIdx.x;
    float *hist = state;
    float *dhist = state + kH;
    for(uint32_t j = t; j < kH; j += kEncThreads) wx[j] = hist[j];
    for(uint32_t j = t; j < kD; j += kEncThreads)
    {
#pragma unroll
        for(int q = 0; q < 4; ++q) dl[q][j] = dhist[q * kD + j];
    }
    for(uint32_t i = t; i < n; i += kEncThreads)
    {
        mix(i, dl[0][kD + i], wx[kH + i], dl[1][kD + i]);
        dl[2][kD + i] = left[i];
        dl[3][kD + i] = right[i];
    }
    __syncthreads();
    for(uint32_t i = t; i < n; i += kEncThreads)
    {
        // jwx[i] = sum_k taps[k] * wx[i - 129 - 2k]: ext index kH + i - 129 - 2k >= 0 for k < N/2
        const float *src = wx + (kH + i - 129u);
        double acc = 0.0;
#pragma unroll 8
        for(uint32_t k = 0; k < N / 2u; ++k) acc = fma(double(taps[k]), double(src[-int(2u * k)]), acc);
        const float jwx = float(acc);
        const float sv = dl[0][i], dv = jwx + yGain * dl[1][i];
        left[i] = dl[2][i] + (sv + dv);
        right[i] = dl[3][i] + (sv - dv);
    }
    // the next update's histories: the last kH / kD samples of [history | update]
    for(uint32_t j = t; j < kH; j += kEncThreads) hist[j] = wx[n + j];
    for(uint32_t j = t; j < kD; j += kEncThreads)
    {
#pragma unroll
        for(int q = 0; q < 4; ++q) dhist[q * kD + j] = dl[q][n + j];
    }
}

constexpr size_t EncFirStateFloats(uint32_t n) { return size_t{n + 127u} + 4u * size_t{n / 2u + 128u}; }

} // namespace oalgpu
