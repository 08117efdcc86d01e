// present.h — the display value of a colour: the arithmetic of RayTracer::Pixels() (RayTracer.cpp:16-18,65-66,
// ToColor(clamp(c, 0, 1))) as one function (DESIGN.md §6g, rt2.h "Presenting reconstructed frames"), callable
// from host and device: the GPU kernel (present.hip), the CPU test program (tests/cpp/present_host.cpp) and the
// numpy statement (tests/present_ref.py) are this arithmetic.
//
// Per channel k of a float32 colour c, only comparisons, selects, one conversion to double, one double multiply,
// floor and one conversion to an integer:
//   v   = c_k > 0 ? c_k : 0          (a comparison with NaN is false: NaN -> 0; -0 -> 0; -inf -> 0)
//   v   = v < 1 ? v : 1              (+inf -> 1)
//   b_k = (uint8_t)floor((double)v * 255.999)
//   PresentPixel(c) = 0xFF000000 | b_0 | b_1 << 8 | b_2 << 16          (the bytes R, G, B, A = 255 in memory)
// v is in [0, 1], so the product is in [0, 255.999]: the conversion never leaves the range of uint8_t and b_k is
// at most 255. The double product of a float32 and 255.999 is rounded once; no float32 below 1 reaches 256.
//
// For every finite channel these are the bytes accumulate_kernel (render.hip) and deinterleave_kernel
// (gather.hip) derive from accum / frame_idx: their clamp max(min) gives the same v. -0 gives byte 0, like glm's
// clamp. Unlike them the function is defined for every input: NaN -> 0, +inf -> 255, -inf -> 0 (a filtered or
// blended pixel that is not finite passes through the reconstruction unchanged, denoise.h / temporal.h, and is
// shown as that).
#ifndef RT2_PRESENT_H_
#define RT2_PRESENT_H_

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RT2_PR_HD __host__ __device__ inline
#else
#define RT2_PR_HD inline
#endif

namespace rt2 {

RT2_PR_HD uint32_t PresentPixel(const float c[3]) {
  uint32_t rgba = 0xFF000000u;
  for (int k = 0; k < 3; k++) {
    float v = c[k] > 0.0f ? c[k] : 0.0f;
    v = v < 1.0f ? v : 1.0f;
    rgba |= ((uint32_t)(uint8_t)floor((double)v * 255.999)) << (8 * k);
  }
  return rgba;
}

}  // namespace rt2

#endif  // RT2_PRESENT_H_
