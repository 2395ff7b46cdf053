// The bs2b crossfeed (Bauer stereophonic-to-binaural): DeviceBase::Process(Bs2bPostProcess) (alc/alu.cpp:407-434) around the
// B-Format decode of a stereo device; bs2b_processor::cross_feed (core/bs2b.cpp:107-163).
//
// Two launches with the unchanged decode between them.  CrossfeedSplitKernel (in front of the decode) moves the direct left and
// right lines out into the context's state and zeroes them, so that the filter sees the decoded feeds alone.  CrossfeedKernel
// (behind it) is one workgroup of four wavefronts per context and update: the two decoded lines are staged in LDS; the four
// first-order recurrences of cross_feed (left high-boost, left low-pass, right low-pass, right high-boost) are four serial
// chains, one lane each on wavefront 0, reading LDS and writing their outputs as [sample][chain] (a lane's stores are four
// words apart from its neighbours': no bank conflict, and the combine reads a sample's four words at once); the combine
// left = hi(L) + lo(R), right = lo(L) + hi(R), + the saved direct line runs 256 samples wide.
//
// Per sample and chain the reference computes y = a0 x + z, then z = a1 x + b1 y (high-boost) or z = b1 y (low-pass), every
// product and sum rounded on its own; the same here, contraction off: bit-identical.  The reference's 128-sample blocks only
// stage data, the histories carry across them.
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace oalgpu {
namespace {

constexpr uint32_t kCfThreads = 256;

__global__ __launch_bounds__(kCfThreads) void CrossfeedSplitKernel(float *left, float *right, float *ldirect, float *rdirect,
    uint32_t n)
{
    for(uint32_t i = threadIdx.x; i < n; i += kCfThreads)
    {
        ldirect[i] = left[i];
        rdirect[i] = right[i];
        left[i] = 0.0f;
        right[i] = 0.0f;
    }
}

// state: history[0].lo, history[0].hi, history[1].lo, history[1].hi | pad to kCrossfeedScratch | the direct left line [1024] |
// the direct right line [1024] (CrossfeedSplitKernel's)
__global__ __launch_bounds__(kCfThreads) void CrossfeedKernel(float *left, float *right, uint32_t n, CrossfeedConsts K,
    float *state)
{
    __shared__ float in[2][kLine];
    __shared__ float out[kLine * 4];           // [sample][hi(L), lo(L), lo(R), hi(R)]
    const uint32_t t = threadIdx.x;
    for(uint32_t i = t; i < n; i += kCfThreads)
    {
        in[0][i] = left[i];
        in[1][i] = right[i];
    }
    __syncthreads();
    if(t < 4u)
    {
        const bool lo = t == 1u || t == 2u;
        const float a0 = lo ? K.a0Lo : K.a0Hi, b1 = lo ? K.b1Lo : K.b1Hi, a1 = K.a1Hi;
        const uint32_t slot = t < 2u ? (t ^ 1u) : t;
        float z = state[slot];
        const float *x = in[t >> 1];
        float *o = out + t;
#pragma unroll 8
        for(uint32_t i = 0; i < n; ++i)
        {
            const float xv = x[i];
            const float y = a0 * xv + z;
            const float by = b1 * y;
            const float hz = a1 * xv + by;
            z = lo ? by : hz;
            o[i * 4u] = y;
        }
        state[slot] = z;
    }
    __syncthreads();
    const float *ldirect = state + kCrossfeedScratch;
    const float *rdirect = ldirect + kLine;
    for(uint32_t i = t; i < n; i += kCfThreads)
    {
        const float *q = out + i * 4u;
        left[i] = (q[0] + q[2]) + ldirect[i];
        right[i] = (q[1] + q[3]) + rdirect[i];
    }
}

} // namespace

void LaunchCrossfeedSplit(hipStream_t s, float *real, uint32_t lidx, uint32_t ridx, uint32_t n, float *state)
{
    float *ldirect = state + kCrossfeedScratch;
    hipLaunchKernelGGL(CrossfeedSplitKernel, dim3(1), dim3(kCfThreads), 0, s, real + size_t{lidx} * kLine,
        real + size_t{ridx} * kLine, ldirect, ldirect + kLine, n);
}

void LaunchCrossfeed(hipStream_t s, float *real, uint32_t lidx, uint32_t ridx, uint32_t n, const CrossfeedConsts &k, float *state)
{
    hipLaunchKernelGGL(CrossfeedKernel, dim3(1), dim3(kCfThreads), 0, s, real + size_t{lidx} * kLine,
        real + size_t{ridx} * kLine, n, k, state);
}

} // namespace oalgpu
