// present.hip — the tone map of present.h on the GPU (rt2.h "Presenting reconstructed frames"):
// the last kernel of a present, on the caller's stream after the blend and the filter.
//
//   present  one thread per pixel: the pixel's float3 colour as the denoise scratch's head holds it (interleaved,
//            three 4-byte loads; a wave reads 768 contiguous bytes) to one RGBA8 word (a wave stores 256
//            contiguous bytes). It reads no other pixel, so there is no LDS stage and no atomic; 12 bytes in and
//            4 out per pixel, nothing to reuse: the kernel runs at the rate memory delivers them.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "present.h"

namespace rt2 {
namespace dev {

constexpr int kPrBlock = 256;

__global__ __launch_bounds__(kPrBlock) void present_kernel(const float* __restrict__ color, uint32_t* __restrict__ rgba,
                                                           uint32_t npix) {
  const uint32_t i = blockIdx.x * (uint32_t)kPrBlock + threadIdx.x;
  if (i >= npix) return;
  const float c[3] = {color[3ull * i], color[3ull * i + 1], color[3ull * i + 2]};
  rgba[i] = PresentPixel(c);
}

}  // namespace dev

// color: npix float3 (device); rgba: npix RGBA8 words (device, 4-byte aligned).
hipError_t LaunchPresent(const float* color, void* rgba, uint32_t npix, hipStream_t stream) {
  if (npix == 0) return hipSuccess;
  const uint32_t blocks = (npix + (uint32_t)dev::kPrBlock - 1u) / (uint32_t)dev::kPrBlock;
  hipLaunchKernelGGL(dev::present_kernel, dim3(blocks), dim3(dev::kPrBlock), 0, stream, color, static_cast<uint32_t*>(rgba),
                     npix);
  return hipGetLastError();
}

}  // namespace rt2
