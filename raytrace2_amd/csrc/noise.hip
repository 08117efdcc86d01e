// noise.hip — standard error of the mean per pixel and the image's noise scalars (rt2.h rt2_noise),
// from the accumulation and the sums of squares accumulate_kernel keeps when moments are on.
//
// One thread per local pixel evaluates noise.h NoiseOfPixel (double arithmetic, the same function the
// host test runs), optionally stores the float3 standard error, and the workgroup reduces its 256
// pixels: across each wave64 with cross-lane operations (a ballot for the two counts, an xor butterfly
// for the sum and the maximum, whose every step adds the same two values in both lanes), then across
// the four waves through LDS in wave order. Each workgroup writes one partial; the host adds the
// partials in block order. No atomics: the same image gives the same bits every time.
// counts (adaptive sampling, else null): each pixel's own sample count n_p in place of n_frames.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "noise.h"

namespace rt2 {
namespace dev {

constexpr int kNoiseBlock = 256;
constexpr int kNoiseWaves = kNoiseBlock / 64;

__global__ __launch_bounds__(kNoiseBlock) void noise_kernel(const float* __restrict__ accum,
                                                            const float* __restrict__ moment2,
                                                            const uint32_t* __restrict__ counts,
                                                            float* __restrict__ sem, NoisePartial* __restrict__ partials,
                                                            uint32_t npix, long long n_frames, double threshold) {
  __shared__ NoisePartial part[kNoiseWaves];
  const uint32_t i = blockIdx.x * (uint32_t)kNoiseBlock + threadIdx.x;
  // lanes past the image take part in the reduction with neutral values
  double sq = 0.0, mx = 0.0;
  bool below = false, bad = false;
  if (i < npix) {
    const float a[3] = {accum[3ull * i], accum[3ull * i + 1], accum[3ull * i + 2]};
    const float q[3] = {moment2[3ull * i], moment2[3ull * i + 1], moment2[3ull * i + 2]};
    const PixelNoise pn = NoiseOfPixel(a, q, counts ? (int64_t)counts[i] : (int64_t)n_frames);
    if (sem) {
      sem[3ull * i] = pn.sem[0];
      sem[3ull * i + 1] = pn.sem[1];
      sem[3ull * i + 2] = pn.sem[2];
    }
    if (pn.finite) {
      sq = pn.err * pn.err;
      mx = pn.err;
      below = pn.err <= threshold;
    } else {
      bad = true;
    }
  }
  const uint64_t n_below = (uint64_t)__popcll(__ballot(below));
  const uint64_t n_bad = (uint64_t)__popcll(__ballot(bad));
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double osq = __shfl_xor(sq, d, 64);
    const double omx = __shfl_xor(mx, d, 64);
    sq = sq + osq;
    mx = omx > mx ? omx : mx;
  }
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) {
    part[wave].sum_sq = sq;
    part[wave].max_err = mx;
    part[wave].below = n_below;
    part[wave].nonfinite = n_bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    NoisePartial r = part[0];
    for (int w = 1; w < kNoiseWaves; w++) {
      r.sum_sq = r.sum_sq + part[w].sum_sq;
      r.max_err = part[w].max_err > r.max_err ? part[w].max_err : r.max_err;
      r.below += part[w].below;
      r.nonfinite += part[w].nonfinite;
    }
    partials[blockIdx.x] = r;
  }
}

}  // namespace dev

uint32_t NoiseBlocks(uint32_t npix) { return (npix + (uint32_t)dev::kNoiseBlock - 1u) / (uint32_t)dev::kNoiseBlock; }

// sem: float3 per pixel, or null; partials: NoiseBlocks(npix) entries.
hipError_t LaunchNoise(const float* accum, const float* moment2, const uint32_t* counts, float* sem,
                       NoisePartial* partials, uint32_t npix, int64_t n_frames, float threshold, hipStream_t stream) {
  if (npix == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::noise_kernel, dim3(NoiseBlocks(npix)), dim3(dev::kNoiseBlock), 0, stream, accum, moment2, counts,
                     sem, partials, npix, (long long)n_frames, (double)threshold);
  return hipGetLastError();
}

}  // namespace rt2
