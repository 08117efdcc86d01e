// gather.hip — root side of the multi-GPU image gather.
//
// Every GPU renders the interleaved row bands of its rank (rt2_layout.h BandRank) into a compact
// band stack; the stacks, padded to the same height, arrive on the root one after another
// ([world][max_rows][W] float3, by ncclGather or device-local copies). This kernel writes them
// back to image order and derives Pixels() = ToColor(clamp(accum / frame_idx, 0, 1))
// (RayTracer.cpp:16-18,65-66) with the same operations as accumulate_kernel, so the gathered image
// is bit-identical to a one-GPU render.
//
// deinterleave_estimate_kernel is the same pass over two stacks, the sums and the sums of squares
// (rt2_tracer_gather_estimate): beside the image it writes the variance of the mean the denoiser takes
// (denoise.h DenoiseVarianceOfSem over noise.h NoiseOfPixel), so the image-order sums of squares are
// never stored.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "rt2_layout.h"

namespace rt2 {
namespace dev {

// glm's scalar min/max (func_common.inl): max(x, y) = x < y ? y : x, min(x, y) = y < x ? y : x
__device__ __forceinline__ float gmax1(float x, float y) { return x < y ? y : x; }
__device__ __forceinline__ float gmin1(float x, float y) { return y < x ? y : x; }

// One thread per image pixel: coalesced reads of one band-stack row, coalesced writes of one image row.
__global__ __launch_bounds__(256) void deinterleave_kernel(const float* __restrict__ stacks, float* __restrict__ image,
                                                           float* __restrict__ image_nc,
                                                           uint32_t* __restrict__ pixels, uint32_t width,
                                                           uint32_t npix, uint32_t band_h, uint32_t world,
                                                           uint32_t max_rows, int frame_idx) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= npix) return;
  const uint32_t y = i / width, x = i - y * width;
  const BandRow src = BandSource((int)y, (int)band_h, (int)world);  // rt2_layout.h
  const float* s = stacks + 3ull * (((unsigned long long)src.rank * max_rows + (uint32_t)src.row) * width + x);
  const float a0 = s[0], a1 = s[1], a2 = s[2];
  image[3ull * i] = a0;
  image[3ull * i + 1] = a1;
  image[3ull * i + 2] = a2;
  // NonConvertedPixels() (RayTracer.cpp:108-109): accumulation / frame_idx_ in float
  const float fi = (float)frame_idx;
  const float cc[3] = {a0 / fi, a1 / fi, a2 / fi};
  image_nc[3ull * i] = cc[0];
  image_nc[3ull * i + 1] = cc[1];
  image_nc[3ull * i + 2] = cc[2];
  uint32_t rgba = 0u;  // Reset() state: nothing rendered yet
  if (frame_idx > 0) {
    rgba = 0xFF000000u;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float v = gmin1(gmax1(cc[k], 0.0f), 1.0f);
      rgba |= ((uint32_t)(uint8_t)floor((double)v * 255.999)) << (8 * k);
    }
  }
  pixels[i] = rgba;
}

// The same over the sums and the sums of squares: deinterleave_kernel's three outputs with its operations,
// and variance[i] = DenoiseVarianceOfSem(NoiseOfPixel(a, q, frame_idx).sem), what denoise_inputs_kernel
// evaluates on a one-GPU tracer. frame_idx >= 2 (the host checks). 24 bytes read and 32 written per pixel.
__global__ __launch_bounds__(256) void deinterleave_estimate_kernel(
    const float* __restrict__ stacks, const float* __restrict__ stacks2, float* __restrict__ image,
    float* __restrict__ image_nc, uint32_t* __restrict__ pixels, float* __restrict__ variance, uint32_t width,
    uint32_t npix, uint32_t band_h, uint32_t world, uint32_t max_rows, int frame_idx) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= npix) return;
  const uint32_t y = i / width, x = i - y * width;
  const BandRow src = BandSource((int)y, (int)band_h, (int)world);  // rt2_layout.h
  const unsigned long long at = 3ull * (((unsigned long long)src.rank * max_rows + (uint32_t)src.row) * width + x);
  const float a[3] = {stacks[at], stacks[at + 1], stacks[at + 2]};
  const float q[3] = {stacks2[at], stacks2[at + 1], stacks2[at + 2]};
  image[3ull * i] = a[0];
  image[3ull * i + 1] = a[1];
  image[3ull * i + 2] = a[2];
  const float fi = (float)frame_idx;
  const float cc[3] = {a[0] / fi, a[1] / fi, a[2] / fi};
  image_nc[3ull * i] = cc[0];
  image_nc[3ull * i + 1] = cc[1];
  image_nc[3ull * i + 2] = cc[2];
  uint32_t rgba = 0xFF000000u;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float v = gmin1(gmax1(cc[k], 0.0f), 1.0f);
    rgba |= ((uint32_t)(uint8_t)floor((double)v * 255.999)) << (8 * k);
  }
  pixels[i] = rgba;
  const PixelNoise pn = NoiseOfPixel(a, q, (int64_t)frame_idx);
  variance[i] = DenoiseVarianceOfSem(pn.sem);
}

// The gather of ranks with adaptive sampling on (rt2.h "Adaptive sampling of the gathered image"): a third stack
// holds each pixel's own sample count n_p, and what the two kernels above divide by (float)frame_idx is divided by
// (float)n_p, with the operations of the one-GPU readbacks: the mean of non_converted_pixels, the pixel of
// accumulate_list_kernel (a pixel no launch has written yet, n_p = 0, keeps the reset's zero word), and with
// kSquares the variance that denoise_inputs_kernel takes from the pixel's own count. n_p goes out in image order
// for the chain's blend lengths and rt2_tracer_image_sample_counts. 16 (kSquares: 28) bytes read and 32 (36)
// written per pixel; the rows of all three stacks are read, and the image rows written, as the kernels above do.
template <bool kSquares>
__global__ __launch_bounds__(256) void deinterleave_adaptive_kernel(
    const float* __restrict__ stacks, const float* __restrict__ stacks2, const uint32_t* __restrict__ counts,
    float* __restrict__ image, float* __restrict__ image_nc, uint32_t* __restrict__ pixels, float* __restrict__ variance,
    uint32_t* __restrict__ image_counts, uint32_t width, uint32_t npix, uint32_t band_h, uint32_t world,
    uint32_t max_rows) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= npix) return;
  const uint32_t y = i / width, x = i - y * width;
  const BandRow src = BandSource((int)y, (int)band_h, (int)world);  // rt2_layout.h
  const unsigned long long from = ((unsigned long long)src.rank * max_rows + (uint32_t)src.row) * width + x;
  const unsigned long long at = 3ull * from;
  const uint32_t n = counts[from];
  const float a[3] = {stacks[at], stacks[at + 1], stacks[at + 2]};
  image[3ull * i] = a[0];
  image[3ull * i + 1] = a[1];
  image[3ull * i + 2] = a[2];
  const float fn = (float)n;
  const float cc[3] = {a[0] / fn, a[1] / fn, a[2] / fn};
  image_nc[3ull * i] = cc[0];
  image_nc[3ull * i + 1] = cc[1];
  image_nc[3ull * i + 2] = cc[2];
  uint32_t rgba = 0u;  // Reset() state: no sample of this pixel yet
  if (n > 0u) {
    rgba = 0xFF000000u;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float v = gmin1(gmax1(cc[k], 0.0f), 1.0f);
      rgba |= ((uint32_t)(uint8_t)floor((double)v * 255.999)) << (8 * k);
    }
  }
  pixels[i] = rgba;
  image_counts[i] = n;
  if constexpr (kSquares) {
    const float q[3] = {stacks2[at], stacks2[at + 1], stacks2[at + 2]};
    const PixelNoise pn = NoiseOfPixel(a, q, (int64_t)n);
    variance[i] = DenoiseVarianceOfSem(pn.sem);
  }
}

}  // namespace dev

hipError_t LaunchDeinterleave(const float* stacks, float* image, float* image_nc, uint8_t* pixels, int width,
                              int height, int band_h, int world, int max_rows, int frame_idx, hipStream_t stream) {
  const uint32_t npix = (uint32_t)width * (uint32_t)height;
  if (npix == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::deinterleave_kernel, dim3((npix + 255u) / 256u), dim3(256), 0, stream, stacks, image,
                     image_nc, reinterpret_cast<uint32_t*>(pixels), (uint32_t)width, npix, (uint32_t)band_h, (uint32_t)world,
                     (uint32_t)max_rows, frame_idx);
  return hipGetLastError();
}

hipError_t LaunchDeinterleaveEstimate(const float* stacks, const float* stacks2, float* image, float* image_nc,
                                      uint8_t* pixels, float* variance, int width, int height, int band_h, int world,
                                      int max_rows, int frame_idx, hipStream_t stream) {
  const uint32_t npix = (uint32_t)width * (uint32_t)height;
  if (npix == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::deinterleave_estimate_kernel, dim3((npix + 255u) / 256u), dim3(256), 0, stream, stacks, stacks2,
                     image, image_nc, reinterpret_cast<uint32_t*>(pixels), variance, (uint32_t)width, npix, (uint32_t)band_h,
                     (uint32_t)world, (uint32_t)max_rows, frame_idx);
  return hipGetLastError();
}

// stacks2 and variance: both given (the estimate's gather), or both null. counts: [world][max_rows][width].
hipError_t LaunchDeinterleaveAdaptive(const float* stacks, const float* stacks2, const uint32_t* counts, float* image,
                                      float* image_nc, uint8_t* pixels, float* variance, uint32_t* image_counts, int width,
                                      int height, int band_h, int world, int max_rows, hipStream_t stream) {
  const uint32_t npix = (uint32_t)width * (uint32_t)height;
  if (npix == 0) return hipSuccess;
  if ((stacks2 == nullptr) != (variance == nullptr)) return hipErrorInvalidValue;
  const auto kernel = stacks2 ? dev::deinterleave_adaptive_kernel<true> : dev::deinterleave_adaptive_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((npix + 255u) / 256u), dim3(256), 0, stream, stacks, stacks2, counts, image, image_nc,
                     reinterpret_cast<uint32_t*>(pixels), variance, image_counts, (uint32_t)width, npix, (uint32_t)band_h,
                     (uint32_t)world, (uint32_t)max_rows);
  return hipGetLastError();
}

}  // namespace rt2
