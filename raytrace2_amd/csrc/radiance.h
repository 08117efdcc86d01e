// radiance.h — radiance queries (include/rt2.h "Radiance queries"): the radiance RayColor returns
// along rays the caller owns. Plain C++ for host and device: the kernels (render.hip radiance_kernel,
// radiance_sum_kernel), the C ABI (capi_query.cpp) and the CPU test program (tests/cpp/radiance_host.cpp) evaluate
// this one text.
//
// Ray record, 8 floats, query.h's: ox oy oz tmax | dx dy dz time. A ray is valid iff QueryRayValid holds; there is
// no second predicate. Each ray has two stream words (pixel word, frame word): streams[i][0..1], or without the
// array (index0 + i, kRadianceFrame0), index0 the index of a chunk's first ray in its call. The default frame word
// is clear of the render's frame indices (below 2^30 in any run that ends) and of ambient.h's 0x80000000 + s.
//
// Sample s of the valid ray i, s in [0, samples):
//   1. open the path stream (seed, pixel word, frame word + s);
//   2. discard its first first_draw uniforms (a camera's own draws: 3, or 5 with defocus);
//   3. run RayColorForward for max_depth on the ray: the first segment's interval is (0.001, tmax), every later
//      one's (0.001, FLT_MAX); the direction is taken as given; a ConstantMedium draws from this same stream; thr
//      starts at (1, 1, 1) and the sample is thr * emission, thr * background, or 0 when the depth runs out.
// out_sum[i] = ((0 + sample_0) + sample_1) + ..., each addition rounded on its own; out_rays[i] = the rays cast,
// RayColor entries with depth > 0, over the samples. An invalid ray answers (0, 0, 0) and kRadianceInvalid.
//
// A (ray, sample) item's result goes to its own slot, 4 words: r g b and the item's ray count; RadianceSum adds a
// ray's slots in sample order onto the running answer, so neither the lane that computed an item nor a split of
// the call over sample ranges can show in the bytes.
#ifndef RT2_RADIANCE_H_
#define RT2_RADIANCE_H_

#include <cstdint>

#include "query.h"

namespace rt2 {

constexpr uint32_t kRadianceFrame0 = 0x40000000u;   // default frame word
constexpr uint32_t kRadianceInvalid = 0xFFFFFFFFu;  // out_rays of an invalid ray
constexpr int kRadianceMaxSamples = 65535;
constexpr int kRadianceMaxDepth = 65535;
constexpr uint32_t kRadianceMaxFirstDraw = 8;
constexpr int kRadianceSlotWords = 4;  // r g b | rays cast

// rt2_radiance_params after defaults and checks, as the kernels take it.
struct RadianceArgs {
  uint32_t samples;     // of the call
  uint32_t max_depth;   // 1..65535 (0 resolved to the tracer's)
  uint32_t first_draw;  // 0..8
};

inline bool RadianceArgsValid(int samples, int max_depth, uint32_t first_draw) {
  return samples >= 1 && samples <= kRadianceMaxSamples && max_depth >= 0 && max_depth <= kRadianceMaxDepth &&
         first_draw <= kRadianceMaxFirstDraw;
}

// frame word + samples must not pass 2^32: sample s opens frame word + s for s < samples.
inline bool RadianceFrameFits(uint32_t frame_word, uint32_t samples) {
  return (uint64_t)frame_word + (uint64_t)samples <= ((uint64_t)1 << 32);
}

RT2_QR_HD bool RadianceRayValid(const float ray[8]) { return QueryRayValid(ray); }

// One launch: the samples [s0, s0 + k) of n rays. Work item w in [0, n * k) is (ray w / k, sample s0 + w % k), the
// sample fastest; its slot is slot w of the launch.
RT2_QR_HD void RadianceItem(uint32_t w, uint32_t k, uint32_t s0, uint32_t* ray, uint32_t* sample) {
  const uint32_t r = w / k;
  *ray = r;
  *sample = s0 + (w - r * k);
}

// The stream words of ray i of a launch.
RT2_QR_HD void RadianceStream(const uint32_t* streams, uint32_t index0, uint32_t i, uint32_t* pixel_word,
                              uint32_t* frame_word) {
  if (streams) {
    *pixel_word = streams[2u * i];
    *frame_word = streams[2u * i + 1u];
  } else {
    *pixel_word = index0 + i;
    *frame_word = kRadianceFrame0;
  }
}

// The ordered sum: a ray's k slots of one launch added onto its running answer (sum3, rays), in sample order.
RT2_QR_HD void RadianceSum(const float* slots, uint32_t k, float sum3[3], uint32_t* rays) {
  float x = sum3[0], y = sum3[1], z = sum3[2];
  uint32_t c = *rays;
  for (uint32_t s = 0; s < k; s++) {
    const float* it = slots + (size_t)kRadianceSlotWords * s;
    x = x + it[0];
    y = y + it[1];
    z = z + it[2];
    c += QueryWord(it[3]);
  }
  sum3[0] = x, sum3[1] = y, sum3[2] = z;
  *rays = c;
}

}  // namespace rt2

#endif  // RT2_RADIANCE_H_
