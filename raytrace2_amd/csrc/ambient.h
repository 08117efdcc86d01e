// ambient.h — ambient occlusion (include/rt2.h "Ambient occlusion"): the rule that turns a surface
// point and a sample index into one occlusion ray. Plain C++ for host and device: the kernel (render.hip
// ambient_kernel), the C ABI (capi_query.cpp rt2_ambient_direction) and the CPU test program
// (tests/cpp/ambient_host.cpp) evaluate this one text.
//
// Point record, 8 floats, the ray record's shape (query.h): px py pz tmax | nx ny nz time. A point is valid iff
// QueryRayValid holds for these eight words, the normal standing in for the direction.
//
// Sample s of the valid point with stream index i, every float operation rounded on its own:
//   u = the first RandUnitVec3 draw of the path stream (seed, pixel word i, frame word kAmbientFrame0 + s)
//   v = n + u                                   per component
//   if every |component of v| <= 1e-8f: v = n   Lambertian scatter's guard (the kernel's near_zero)
//   d = v * (1 / sqrt((vx vx + vy vy) + vz vz)) glm::normalize, the kernel's normalize
// The ray is (p, tmax | d, time), traced as an occlusion query traces that record: interval (0.001, tmax), media
// drawing from the probe stream. A built ray that fails QueryRayValid is masked and counts as clear. The count of
// a point is the number of its occluded samples; an invalid point answers kAmbientInvalid.
// The frame words start above every render frame index, so no render draw is taken again.
// dot(d, n) may be slightly negative where n is not unit: nothing here assumes it is >= 0.
#ifndef RT2_AMBIENT_H_
#define RT2_AMBIENT_H_

#include <cmath>
#include <cstdint>

#include "query.h"

namespace rt2 {

constexpr uint32_t kAmbientFrame0 = 0x80000000u;   // frame word of sample 0
constexpr uint32_t kAmbientInvalid = 0xFFFFFFFFu;  // the count of an invalid point (image mode: of a miss pixel)
constexpr int kAmbientMaxSamples = 65535;
// Feature records as points (rt2.h "Feature buffers and denoiser"): 16 floats, point in 2-4, normal in 5-7
constexpr uint32_t kAmbientFeatureStride = 16, kAmbientFeaturePoint = 2, kAmbientFeatureNormal = 5;
// Caller records as points: the ray record's layout
constexpr uint32_t kAmbientRecordStride = 8, kAmbientRecordPoint = 0, kAmbientRecordNormal = 4;

// Where a launch's points lie on the device: `stride` words per point, the position at off_p, the normal at off_n.
// Feature records take tmax = radius and time 0 and answer kAmbientInvalid where slot 0 is 0 (a miss); width: the
// image's, for the map from a local pixel to its global index. Caller records carry tmax and time (width 0);
// index0: the stream index of the first one (a chunk of a larger call).
struct AmbientSource {
  const float* recs;
  uint32_t stride, off_p, off_n;
  float radius;
  uint32_t width, index0;
};
inline AmbientSource AmbientFeatureSource(const float* d_features, float radius, uint32_t width) {
  return AmbientSource{d_features, kAmbientFeatureStride, kAmbientFeaturePoint, kAmbientFeatureNormal, radius, width, 0u};
}
inline AmbientSource AmbientRecordSource(const float* d_points, uint32_t index0) {
  return AmbientSource{d_points, kAmbientRecordStride, kAmbientRecordPoint, kAmbientRecordNormal, 0.0f, 0u, index0};
}

RT2_QR_HD bool AmbientNearZero(const float v[3]) {
  return QueryAbs(v[0]) <= 1e-8f && QueryAbs(v[1]) <= 1e-8f && QueryAbs(v[2]) <= 1e-8f;
}

// d of the rule above from the normal n and the unit-vector draw u.
RT2_QR_HD void AmbientDirection(const float n[3], const float u[3], float d[3]) {
  float v[3] = {n[0] + u[0], n[1] + u[1], n[2] + u[2]};
  if (AmbientNearZero(v)) v[0] = n[0], v[1] = n[1], v[2] = n[2];
  const float xx = v[0] * v[0], yy = v[1] * v[1], zz = v[2] * v[2];
  const float l2 = (xx + yy) + zz;
  const float inv = 1.0f / sqrtf(l2);
  d[0] = v[0] * inv, d[1] = v[1] * inv, d[2] = v[2] * inv;
}

// The ray record of a sample: the point's origin, tmax and time with d for the normal.
RT2_QR_HD void AmbientRay(const float point[8], const float u[3], float ray[8]) {
  ray[kQrOx] = point[kQrOx], ray[kQrOy] = point[kQrOy], ray[kQrOz] = point[kQrOz], ray[kQrTmax] = point[kQrTmax];
  AmbientDirection(point + kQrDx, u, ray + kQrDx);
  ray[kQrTime] = point[kQrTime];
}

}  // namespace rt2

#endif  // RT2_AMBIENT_H_
