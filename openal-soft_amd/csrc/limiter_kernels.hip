// The device's output limiter: Compressor::process (core/mastering.cpp) over the output lines, one workgroup of four
// wavefronts per context and update.  Everything that does not depend on the compressor's carried state runs 256 samples
// wide -- pre-gain, the linked side chain (max over the lines of |x|), the logs, the sliding hold, the crest factor's
// quotients and exps, the final exps, the look-ahead delay and the apply; the two recurrences (the crest detector's squared
// peak / RMS pair and gainCompressor's (y_1, y_L, c_dev)) run on wavefront 0, 64 samples' inputs fetched at once and broadcast
// with v_readlane, as WaveSerial does (effects_dev.hpp).
//
// The sliding hold (UpdateSlidingHold / ShiftSlidingHold, Harter's descending maxima) is exactly the maximum of the last
// `hold` log values, the update's and the ones before it (an entry written at i expires at i + hold; the -inf it starts with
// loses to any log value): here a sparse table over [the last hold - 1 values | this update's], bit-identical since max is exact.
//
// logf / expf are the correctly rounded float of the double-precision result; glibc's are not in the last bit for a few
// inputs, so parity with the compiled reference is bounded, not bit-exact.
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace oalgpu {
namespace {

constexpr uint32_t kLimThreads = 256;

__device__ __forceinline__ float MaxRef(float a, float b) { return (a < b) ? b : a; }               // std::max(a, b)
__device__ __forceinline__ float LerpRef(float v1, float v2, float mu) { return v1 + (v2 - v1) * mu; }   // lerpf, alnumeric.h
__device__ __forceinline__ float ExpRounded(float x) { return float(exp(double(x))); }
__device__ __forceinline__ float LogRounded(float x) { return float(log(double(x))); }

// step(x, i) for i = 0 .. n-1 IN ORDER on one wavefront; load(i, v) fetches sample i's NV inputs, 64 samples at once
template<int NV, typename Load, typename Step>
__device__ __forceinline__ void SerialOnWave(uint32_t n, uint32_t lane, Load &&load, Step &&step)
{
    float next[NV];
    load(lane < n ? lane : n - 1u, next);
    for(uint32_t base = 0; base < n; base += 64u)
    {
        float v[NV];
#pragma unroll
        for(int q = 0; q < NV; ++q) v[q] = next[q];
        // the next round's inputs are in flight while this one's samples go through the chain (they are not what it writes)
        if(base + 64u < n) load(base + 64u + lane < n ? base + 64u + lane : n - 1u, next);
        const uint32_t cnt = __builtin_amdgcn_readfirstlane((n - base) < 64u ? (n - base) : 64u);
        if(cnt == 64u)
        {
#pragma unroll
            for(int k = 0; k < 64; ++k)
            {
                float x[NV];
#pragma unroll
                for(int q = 0; q < NV; ++q) x[q] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[q]), k));
                step(x, base + uint32_t(k));
            }
        }
        else
        {
            for(uint32_t k = 0; k < cnt; ++k)
            {
                const int kk = int(__builtin_amdgcn_readfirstlane(k));
                float x[NV];
#pragma unroll
                for(int q = 0; q < NV; ++q) x[q] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[q]), kk));
                step(x, base + k);
            }
        }
    }
}

// state: [0..4] the carried scalars (mLastPeakSq, mLastRmsSq, mLastRelease, mLastAttack, mLastGainDev) | pad to 16 |
// [16, 16 + 1024) the side chain's look-ahead tail | [1040, 2064) the last hold - 1 log values | 7 x 1024 of scratch |
// the delay lines, 1024 each.
// The scratch is device memory, not LDS: the resident HRTF voice kernel leaves a CU 3 KB of LDS, and the limiter has to find room
// beside it (the next update's reduction waits for the limiter).  One workgroup, so __syncthreads orders it.
__global__ __launch_bounds__(kLimThreads) void LimiterKernel(float *lines, uint32_t n, LimiterConsts K, float *state)
{
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    float *carry = state;
    float *tail = state + 16;
    float *holdHist = state + 16 + kLine;
    float *scratch = state + 16 + 2 * kLine;
    float *A = scratch, *B = scratch + 2 * kLine;      // the hold's sparse table (ping-pong); the extended side chain; the delay staging
    float *P = scratch + 4 * kLine;                   // side chain -> x_over -> postGain - y_L -> gains
    float *Q = P + kLine, *R = Q + kLine;             // squared peak -> a_att; squared RMS -> a_rel
    float *delay = scratch + 7 * kLine;
    const uint32_t nch = K.numChans, LA = K.lookAhead, H = K.hold;
    const bool crest = (K.flags & (kLimAutoAttack | kLimAutoRelease)) != 0;
    const float preGain = K.preGain;

    // pre-gain and the linked side chain
    for(uint32_t i = t; i < n; i += kLimThreads)
    {
        float m = 0.0f;
        for(uint32_t c = 0; c < nch; ++c)
        {
            float x = lines[size_t{c} * kLine + i];
            if(preGain != 1.0f) x = x * preGain;
            m = MaxRef(m, fabsf(x));
        }
        P[i] = m;
    }
    __syncthreads();

    // the crest detector (wavefront 0) beside the logs (the others; all four without automated attack / release)
    const uint32_t Hm1 = H ? H - 1u : 0u;
    float *S = A;                                     // the extended side chain: [look-ahead tail | this update's held logs]
    if(crest && wave == 0)
    {
        const float a_crest = K.crestCoeff;
        float y2_peak = carry[0], y2_rms = carry[1];
        SerialOnWave<1>(n, lane, [&](uint32_t i, float *v) {
            const float x_abs = P[i];
            const float sq = x_abs * x_abs;
            v[0] = (sq < 0.000001f) ? 0.000001f : (1000000.0f < sq) ? 1000000.0f : sq;     // std::clamp
        }, [&](const float *x, uint32_t i) {
            const float x2 = x[0];
            y2_peak = MaxRef(x2, LerpRef(x2, y2_peak, a_crest));
            y2_rms = LerpRef(x2, y2_rms, a_crest);
            Q[i] = y2_peak; R[i] = y2_rms;              // (every lane holds the same values: one store each)
        });
        if(lane == 0) { carry[0] = y2_peak; carry[1] = y2_rms; }
    }
    else
    {
        const uint32_t first = crest ? 64u : 0u, stride = kLimThreads - first, u = t - first;
        for(uint32_t i = u; i < n; i += stride)
        {
            const float lg = LogRounded(MaxRef(0.000001f, P[i]));
            if(H) A[Hm1 + i] = lg; else A[LA + i] = lg;
        }
        if(H) { for(uint32_t j = u; j < Hm1; j += stride) A[j] = holdHist[j]; }
        else { for(uint32_t j = u; j < LA; j += stride) A[j] = tail[j]; }
    }
    __syncthreads();

    if(H)
    {   // the sliding hold: cur[j] = max(ext[j .. j + w)), doubling w while 2w <= H; held[i] = max over ext[i .. i + H)
        const uint32_t m = Hm1 + n;
        for(uint32_t j = t; j < Hm1; j += kLimThreads) holdHist[j] = A[n + j];      // the next update's history
        float *cur = A, *nxt = B;
        uint32_t w = 1u;
        for(; 2u * w <= H; w *= 2u)
        {
            for(uint32_t j = t; j + 2u * w <= m; j += kLimThreads) nxt[j] = MaxRef(cur[j], cur[j + w]);
            __syncthreads();
            float *sw = cur; cur = nxt; nxt = sw;
        }
        S = nxt;
        for(uint32_t i = t; i < n; i += kLimThreads) S[LA + i] = MaxRef(cur[i], cur[i + H - w]);
        for(uint32_t j = t; j < LA; j += kLimThreads) S[j] = tail[j];
        __syncthreads();
    }

    // what the gain chain takes per sample and does not depend on its state: x_over, a_att, a_rel
    {
        const float attack = K.attack, release = K.release, threshold = K.threshold;
        const bool autoAttack = (K.flags & kLimAutoAttack) != 0, autoRelease = (K.flags & kLimAutoRelease) != 0;
        for(uint32_t i = t; i < n; i += kLimThreads)
        {
            P[i] = S[LA + i] - threshold;
            if(!crest) continue;
            const float y2_crest = Q[i] / R[i];
            float t_att = attack, a_att = K.attackCoeff, a_rel = K.releaseCoeff;
            if(autoAttack)
            {
                t_att = 2.0f * attack / y2_crest;
                a_att = ExpRounded(-1.0f / t_att);
            }
            if(autoRelease)
            {
                const float t_rel = 2.0f * release / y2_crest - t_att;
                a_rel = ExpRounded(-1.0f / t_rel);
            }
            Q[i] = a_att; R[i] = a_rel;
        }
    }
    __syncthreads();

    // gainCompressor's recurrence (wavefront 0): P[i] <- postGain - y_L; the others move the look-ahead tail on
    if(wave == 0)
    {
        const bool autoKnee = (K.flags & kLimAutoKnee) != 0, autoPostGain = (K.flags & kLimAutoPostGain) != 0;
        const bool autoDeclip = (K.flags & kLimAutoDeclip) != 0;
        const float threshold = K.threshold, slope = K.slope, c_est = K.gainEstimate, a_adp = K.adaptCoeff;
        const float aAtt0 = K.attackCoeff, aRel0 = K.releaseCoeff;
        float postGain = K.postGain, knee = K.knee;
        float y_1 = carry[2], y_L = carry[3], c_dev = carry[4];
        SerialOnWave<4>(n, lane, [&](uint32_t i, float *v) {
            v[0] = P[i]; v[1] = S[i];
            v[2] = crest ? Q[i] : aAtt0; v[3] = crest ? R[i] : aRel0;
        }, [&](const float *x, uint32_t i) {
            const float x_over = x[0], input = x[1], a_att = x[2], a_rel = x[3];
            if(autoKnee) knee = MaxRef(0.0f, 2.5f * (c_dev + c_est));
            const float knee_h = 0.5f * knee;
            const float y_G = (x_over <= -knee_h) ? 0.0f
                : (fabsf(x_over) < knee_h) ? (x_over + knee_h) * (x_over + knee_h) / (2.0f * knee)
                : x_over;
            const float x_L = -slope * y_G;
            y_1 = MaxRef(x_L, LerpRef(x_L, y_1, a_rel));
            y_L = LerpRef(y_1, y_L, a_att);
            c_dev = LerpRef(-(y_L + c_est), c_dev, a_adp);
            if(autoPostGain)
            {
                if(autoDeclip) c_dev = MaxRef(c_dev, input - y_L - threshold - c_est);
                postGain = -(c_dev + c_est);
            }
            P[i] = postGain - y_L;
        });
        if(lane == 0) { carry[2] = y_1; carry[3] = y_L; carry[4] = c_dev; }
    }
    else
    {
        for(uint32_t j = t - 64u; j < LA; j += kLimThreads - 64u) tail[j] = S[n + j];
    }
    __syncthreads();
    for(uint32_t i = t; i < n; i += kLimThreads) P[i] = ExpRounded(P[i]);
    __syncthreads();

    // the look-ahead delay and the apply, line by line: [delay line | the update's samples] staged in the side chain's buffer
    float *C = S;
    for(uint32_t c = 0; c < nch; ++c)
    {
        float *line = lines + size_t{c} * kLine;
        if(LA == 0)
        {
            for(uint32_t i = t; i < n; i += kLimThreads)
            {
                float x = line[i];
                if(preGain != 1.0f) x = x * preGain;
                line[i] = P[i] * x;
            }
            continue;
        }
        float *dl = delay + size_t{c} * kLine;
        for(uint32_t j = t; j < LA + n; j += kLimThreads)
        {
            float x;
            if(j < LA) x = dl[j];
            else { x = line[j - LA]; if(preGain != 1.0f) x = x * preGain; }
            C[j] = x;
        }
        __syncthreads();
        for(uint32_t i = t; i < n; i += kLimThreads) line[i] = P[i] * C[i];
        for(uint32_t j = t; j < LA; j += kLimThreads) dl[j] = C[n + j];
        __syncthreads();
    }
}

} // namespace

void LaunchLimiter(hipStream_t s, float *lines, uint32_t n, const LimiterConsts &k, float *state)
{
    hipLaunchKernelGGL(LimiterKernel, dim3(1), dim3(kLimThreads), 0, s, lines, n, k, state);
}

size_t LimiterStateFloats(uint32_t nch) { return 16u + 9u * size_t{kLine} + size_t{nch} * kLine; }

} // namespace oalgpu
