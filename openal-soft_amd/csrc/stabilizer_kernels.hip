// The front stabilizer: DeviceBase::Process(StablizerPostProcess) (alc/alu.cpp:329-405) around the B-Format decode, and
// speaker distance compensation: ApplyDistanceComp (alc/alu.cpp:2276-2307).
//
// The stabilizer is two launches with the unchanged decode between them.  StabilizerSplitKernel (in front of the decode) moves
// the direct L / R signal out: mid = L + R, side = L - R into the context's scratch, L = R = 0.  StabilizerKernel (behind it)
// does the rest, one workgroup of four wavefronts per context and update, in 64-sample tiles.
//
// The recurrences are numReal + 2 independent serial chains: BandSplitter::processAllPass of every real line (the direct mid in
// place of line `left`, the direct + decoded side in place of line `right`) and BandSplitter::process of the decoded mid, whose
// all-pass and two-stage low-pass do not depend on each other.  The all-passes take one lane each on wavefront 0; the low-pass
// runs alone on wavefront 1 (on a wavefront of its own it costs the all-pass lanes nothing: in one wavefront the two bodies
// would run one after the other at every step).  The reference's operations in its order, contraction off: bit-identical.
//
// A tile's chain inputs are fetched from global memory into registers by all four wavefronts one tile ahead (the sample-wide
// sums side += L - R and L + R are made on the way), stored to LDS as [sample][chain] with an odd row stride (the chains' lanes
// read a row's consecutive words, a wavefront stores one chain's 64 samples 37 words apart: neither conflicts), filtered in
// place, and combined (alu.cpp:389-404) and written out by wavefronts 2-3 while the chains work on the next tile.  No global
// load sits on a dependent chain.
//
// DistanceCompKernel: out[t] = gain * x[t - delay] per line, the last `delay` inputs carried in the context's state; one
// workgroup per line, every read before the first write (the operation is in place); a line with delay 0 is left alone, its
// gain is NOT applied (ApplyDistanceComp returns before the scale where the delay buffer is empty).
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace oalgpu {
namespace {

constexpr uint32_t kStabThreads = 256;
constexpr uint32_t kTile = 64;                     // samples per tile
constexpr uint32_t kStabChains = 32 + 2;           // the real lines' all-passes, the mid filter's all-pass and its low-pass
constexpr uint32_t kStabLoads = (kStabChains + 3) / 4;   // columns per wavefront
constexpr uint32_t kRow = 37;                      // floats per sample row: odd and >= 4 * kStabLoads

// One chain over its column of a tile, in place: p[k * kRow] = step(p[k * kRow]) for k = 0 .. cnt-1 IN ORDER, eight samples per
// round with the next round's eight read from LDS while this round's go through the chain
template<typename Step>
__device__ __forceinline__ void ChainTile(float *p, uint32_t cnt, bool store, Step &&step)
{
    float nx[8];
    if(cnt >= 8u)
    {
#pragma unroll
        for(uint32_t u = 0; u < 8u; ++u) nx[u] = p[u * kRow];
    }
    uint32_t k = 0;
    for(; k + 8u <= cnt; k += 8u)
    {
        float x[8];
#pragma unroll
        for(uint32_t u = 0; u < 8u; ++u) x[u] = nx[u];
        // (without a branch, so that the reads stay in flight: past the tile's end its last row again, never used)
#pragma unroll
        for(uint32_t u = 0; u < 8u; ++u) nx[u] = p[(k + 8u + u < kTile ? k + 8u + u : kTile - 1u) * kRow];
#pragma unroll
        for(uint32_t u = 0; u < 8u; ++u) x[u] = step(x[u]);
        if(store)
        {
#pragma unroll
            for(uint32_t u = 0; u < 8u; ++u) p[(k + u) * kRow] = x[u];
        }
    }
    for(; k < cnt; ++k)
    {
        const float y = step(p[k * kRow]);
        if(store) p[k * kRow] = y;
    }
}

__global__ __launch_bounds__(kStabThreads) void StabilizerSplitKernel(float *left, float *right, float *mid, float *side,
    uint32_t n)
{
    for(uint32_t i = threadIdx.x; i < n; i += kStabThreads)
    {
        const float l = left[i], r = right[i];
        mid[i] = l + r;
        side[i] = l - r;
        left[i] = 0.0f;
        right[i] = 0.0f;
    }
}

// state: [0, 32) ChannelFilters[i].mApZ1 | [32] MidFilter.mLpZ1, [33] mLpZ2, [34] mApZ1 | pad to kStabilizerScratch | mid[1024]
// | side[1024] (StabilizerSplitKernel's)
__global__ __launch_bounds__(kStabThreads) void StabilizerKernel(float *real, uint32_t numReal, uint32_t lidx, uint32_t ridx,
    uint32_t cidx, uint32_t n, StabilizerConsts K, float *state)
{
    __shared__ float tile[2][kTile * kRow];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const float *mid = state + kStabilizerScratch;
    const float *side = mid + kLine;
    float *leftLine = real + size_t{lidx} * kLine;
    float *rightLine = real + size_t{ridx} * kLine;
    // (chain numReal: the mid filter's all-pass; numReal + 1: its low-pass)
    const uint32_t tiles = (n + kTile - 1u) / kTile;

    // What the chains filter, sample base + lane.  Wavefront w fetches and stores the columns c = q * 4 + w: first every column as
    // the plain line (past the last line: the last line again, never used), then, in the same wavefront and so behind them in
    // LDS order, the four columns that hold something else: mid, side, and the decoded mid twice.  Past the update's end a tile
    // repeats its last sample.  No branch, no select: the loads go out back to back.
    float next[kStabLoads], nextMid, nextSide, nextSum;
    auto fetch = [&](uint32_t base) {
        const uint32_t i = base + lane < n ? base + lane : n - 1u;
        const float l = leftLine[i], r = rightLine[i];
        nextMid = mid[i];
        nextSide = side[i] + (l - r);
        nextSum = l + r;
#pragma unroll
        for(uint32_t q = 0; q < kStabLoads; ++q)
        {
            const uint32_t c = q * 4u + wave;
            next[q] = real[size_t{c < numReal - 1u ? c : numReal - 1u} * kLine + i];
        }
    };

    // the chains' carried state: lane c of wavefront 0 its all-pass z1; lane 0 of wavefront 1 the low-pass pair
    const float coeff = K.coeff;
    const float lpCoeff = coeff * 0.5f + 0.5f;
    float z1 = 0.0f, z2 = 0.0f;
    if(wave == 0 && lane <= numReal) z1 = lane < numReal ? state[lane] : state[34];
    if(wave == 1) { z1 = state[32]; z2 = state[33]; }

    fetch(0u);
    for(uint32_t j = 0; j <= tiles; ++j)
    {
        float *cur = tile[j & 1u];
        if(j < tiles)
        {
            float *row = cur + lane * kRow;
#pragma unroll
            for(uint32_t q = 0; q < kStabLoads; ++q) row[q * 4u + wave] = next[q];
            if((lidx & 3u) == wave) row[lidx] = nextMid;
            if((ridx & 3u) == wave) row[ridx] = nextSide;
            if((numReal & 3u) == wave) row[numReal] = nextSum;
            if(((numReal + 1u) & 3u) == wave) row[numReal + 1u] = nextSum;
        }
        __syncthreads();
        // the next tile's inputs are in flight while this one's go through the chains
        if(j + 1u < tiles) fetch((j + 1u) * kTile);
        const uint32_t cnt = j < tiles ? ((n - j * kTile) < kTile ? (n - j * kTile) : kTile) : 0u;
        if(wave == 0)
        {
            if(lane <= numReal)
            {   // BandSplitter::processAllPass (and the all-pass half of ::process)
                ChainTile(cur + lane, cnt, true, [&](float x) {
                    const float y = x * coeff + z1;
                    z1 = x - y * coeff;
                    return y;
                });
            }
        }
        else if(wave == 1)
        {   // the low-pass half of BandSplitter::process (every lane computes the same; lane 0 stores)
            ChainTile(cur + (numReal + 1u), cnt, lane == 0, [&](float x) {
                const float d0 = (x - z1) * lpCoeff;
                const float y0 = z1 + d0;
                z1 = y0 + d0;
                const float d1 = (y0 - z2) * lpCoeff;
                const float y1 = z2 + d1;
                z2 = y1 + d1;
                return y1;
            });
        }
        else if(j > 0)
        {   // the combine of the tile before (alu.cpp:389-404) and its way out: line c, sample base + k
            const float *done = tile[(j - 1u) & 1u];
            const uint32_t base = (j - 1u) * kTile;
            const uint32_t u = t - 128u;
            for(uint32_t e = u; e < numReal * kTile; e += 128u)
            {
                const uint32_t c = e >> 6, k = e & 63u;
                if(base + k >= n) continue;
                const float *row = done + k * kRow;
                float v = row[c];
                if(c == lidx || c == ridx || c == cidx)
                {
                    const float lf = row[numReal + 1u];
                    const float hf = row[numReal] - lf;             // MidHF: ap_y - lp_y1
                    if(c == cidx) v = v + (lf * K.centerLf + hf * K.centerHf) * 0.5f;
                    else
                    {
                        const float m = lf * K.midLf + hf * K.midHf + row[lidx];
                        const float s = row[ridx];
                        v = c == lidx ? (m + s) * 0.5f : (m - s) * 0.5f;
                    }
                }
                real[size_t{c} * kLine + base + k] = v;
            }
        }
        __syncthreads();
    }
    if(wave == 0 && lane <= numReal) state[lane < numReal ? lane : 34u] = z1;
    if(wave == 1 && lane == 0) { state[32] = z1; state[33] = z2; }
}

constexpr uint32_t kDistThreads = 256;

// hist: [line][1024], the line's last `delay` inputs in its first `delay` floats
__global__ __launch_bounds__(kDistThreads) void DistanceCompKernel(float *lines, uint32_t n, const uint32_t *delays,
    const float *gains, float *hist)
{
    const uint32_t d = delays[blockIdx.x];
    if(d == 0u) return;
    const float gain = gains[blockIdx.x];
    float *x = lines + size_t{blockIdx.x} * kLine;
    float *h = hist + size_t{blockIdx.x} * kLine;
    const uint32_t t = threadIdx.x;
    // the extended sequence [history | this update's]: out[i] = gain * ext[i], the next history = ext[n + j]
    float out[kLine / kDistThreads], keep[kLine / kDistThreads];
#pragma unroll
    for(uint32_t q = 0; q < kLine / kDistThreads; ++q)
    {
        const uint32_t i = q * kDistThreads + t;
        out[q] = i < n ? (i < d ? h[i] : x[i - d]) : 0.0f;
        const uint32_t e = n + i;
        keep[q] = i < d ? (e < d ? h[e] : x[e - d]) : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for(uint32_t q = 0; q < kLine / kDistThreads; ++q)
    {
        const uint32_t i = q * kDistThreads + t;
        if(i < n) x[i] = out[q] * gain;
        if(i < d) h[i] = keep[q];
    }
}

} // namespace

void LaunchStabilizerSplit(hipStream_t s, float *real, uint32_t lidx, uint32_t ridx, uint32_t n, float *state)
{
    float *mid = state + kStabilizerScratch;
    hipLaunchKernelGGL(StabilizerSplitKernel, dim3(1), dim3(kStabThreads), 0, s, real + size_t{lidx} * kLine,
        real + size_t{ridx} * kLine, mid, mid + kLine, n);
}

void LaunchStabilizer(hipStream_t s, float *real, uint32_t numReal, uint32_t lidx, uint32_t ridx, uint32_t cidx, uint32_t n,
    const StabilizerConsts &k, float *state)
{
    hipLaunchKernelGGL(StabilizerKernel, dim3(1), dim3(kStabThreads), 0, s, real, numReal, lidx, ridx, cidx, n, k, state);
}

void LaunchDistanceComp(hipStream_t s, float *lines, uint32_t nlines, uint32_t n, const uint32_t *delays, const float *gains,
    float *hist)
{
    hipLaunchKernelGGL(DistanceCompKernel, dim3(nlines), dim3(kDistThreads), 0, s, lines, n, delays, gains, hist);
}

} // namespace oalgpu
