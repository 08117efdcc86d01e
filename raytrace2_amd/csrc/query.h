// query.h — ray queries (include/rt2.h "Ray queries"): the record layouts of a caller's ray and
// of its answer, and the rule that says which rays are traced. Plain C++ for host and device: the kernel
// (render.hip query_kernel), the C ABI (capi_query.cpp rt2_query_ray_valid) and the CPU test program
// (tests/cpp/query_host.cpp) evaluate this one predicate.
//
// Ray record, 8 floats (two 16-byte words): ox oy oz tmax | dx dy dz time. The interval is (0.001, tmax): tmin is
// the reference's 0.001 as everywhere in the kernels, FLT_MAX is "unbounded" (kInfinity, Defs.hpp:17). The
// direction is taken as given, not normalised: t is in units of |d|, as Hit sees it.
//
// Hit record, 16 floats, the feature record's layout (rt2.h "Feature buffers and denoiser"):
//   0      1 hit, 0 miss, -1 not traced (QueryRayValid false)
//   1      t (model-space under a transformed child, Transform.cpp:82)
//   2-4    point            5-7  normal, facing against the ray        8  front_face        9  material index
//   10-12  albedo by the feature pass's rule            13  dist = sqrt(dot(point - o, point - o))
//   14-15  0
// A miss: slot 0 = 0, the background in 10-12, 0 elsewhere. Not traced: slot 0 = -1, 0 elsewhere.
//
// QueryRayValid: all eight words finite, 0.001 < tmax, 0 <= time <= 1, and origin and direction inside the domain
// on which the kernels' exact shortcuts are proven (the constants below). A ray outside it never enters a
// traversal loop, which is what makes NaN or garbage input harmless.
#ifndef RT2_QUERY_H_
#define RT2_QUERY_H_

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RT2_QR_HD __host__ __device__ inline
#else
#define RT2_QR_HD inline
#endif

namespace rt2 {

constexpr int kQueryRayFloats = 8;
constexpr int kQueryHitFloats = 16;
// Slots of the ray record
enum QueryRayWord : int { kQrOx = 0, kQrOy = 1, kQrOz = 2, kQrTmax = 3, kQrDx = 4, kQrDy = 5, kQrDz = 6, kQrTime = 7 };

constexpr float kQueryTmin = 0.001f;  // Interval{0.001, .} (render.hip trace_stack / trace_linear `tmin`)

// Origins: every coordinate within +-2^64. capi.cpp:726-736 CameraOriginsBounded ("camera rays start within
// +-2^64 on every axis"): the bound under which the threaded program's rectangle test (compile.cpp:104-109
// RectAAWords: exact for ray origins within +-2^100) holds in every transform's space of a scene within +-2^64
// (compile.cpp:598-625 QuadAASpace), and under which the transforms about y may leave out their +-0 products
// (finite coordinates, compile.cpp YAxisPattern). A query's origin is held to what a camera's is.
constexpr float kQueryOriginMax = 0x1p64f;

// Directions: the largest of |dx|, |dy|, |dz| within [2^-20, 2^20]. render.hip:3443-3447 (rt2_selftest 8) draws
// its directions at the scales 2^-20 .. 2^20: the widest range of direction lengths any of the kernels' statements
// covers. Inside it the other shortcuts hold by their own statements:
//  * div_by_inv (render.hip:860-868) equals IEEE a / b for every pair of significands (rt2_selftest 6 and 7; the
//    algorithm scales exactly with the exponents) whenever no intermediate under- or overflows. Divisors are ray
//    direction components b with 1e-8 < |b| (smaller ones are rejected before t is used, Quad.cpp:22) and here
//    |b| <= 2^20; numerators are plane offsets a = sD - o_K with |a| <= 2^65 by the origin bound. The reciprocal
//    is normal (2^-20 <= |1/b| < 2^27), the quotient is below 2^92, and for the numerators of rt2_selftest 3's range
//    (render.hip:3357: 2^-100 <= |a|) the quotient stays above 2^-120 and the residual a - b q, a multiple of
//    ulp(b) ulp(q) >= 2^-48 |a| >= 2^-148, is exact whatever |b| is: the margins are those at rt2_selftest 0
//    and 3's divisors (render.hip:3358, 3365: |b| < 4), which bound the residual by the numerator alone.
//    A quotient below 0.001 is rejected by the interval whatever its last bit.
//  * recip3 and normalize (render.hip:133-144) check their own ranges and take IEEE division outside them;
//    sphere_t_rec checks sphere_fast_ok_pos (a = dot(d, d) within [2^-60, 2^60]: 2^-40 <= a <= 3 * 2^40 here).
//  * the box-level test's offsets (tests/cpp/box_cert.cpp, tests/cpp/quadaa_bounds.cpp:105-106: origins within
//    +-2^100) depend on the origin alone; its margin is relative to |o| + |d| |t| (boxaa.h:71).
// Unit directions (largest component >= 1/sqrt(3)) and the un-normalised pixel-centre rays pc - center of every
// shipped scene's camera (lengths of the order of focus_distance, 1 .. 1000) lie well inside.
constexpr float kQueryDirMaxLow = 0x1p-20f;
constexpr float kQueryDirMaxHigh = 0x1p20f;

// The launch's workgroups of `block` lanes over n rays rounded up to whole waves (n < 2^31: no product overflows).
inline uint32_t QueryGrid(uint32_t n, uint32_t block) {
  const uint32_t lanes = (n + 63u) & ~63u;
  return (lanes + block - 1u) / block;
}

RT2_QR_HD uint32_t QueryWord(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
RT2_QR_HD bool QueryFinite(float f) { return (QueryWord(f) & 0x7F800000u) != 0x7F800000u; }
RT2_QR_HD float QueryAbs(float f) {
  const uint32_t u = QueryWord(f) & 0x7FFFFFFFu;
  float r;
  memcpy(&r, &u, 4);
  return r;
}

RT2_QR_HD bool QueryRayValid(const float ray[8]) {
  bool ok = true;
  for (int k = 0; k < kQueryRayFloats; k++) ok = ok && QueryFinite(ray[k]);
  const float ax = QueryAbs(ray[kQrDx]), ay = QueryAbs(ray[kQrDy]), az = QueryAbs(ray[kQrDz]);
  float m = ax > ay ? ax : ay;
  m = m > az ? m : az;
  ok = ok && m >= kQueryDirMaxLow && m <= kQueryDirMaxHigh;  // (d != 0 with it)
  ok = ok && QueryAbs(ray[kQrOx]) <= kQueryOriginMax && QueryAbs(ray[kQrOy]) <= kQueryOriginMax &&
       QueryAbs(ray[kQrOz]) <= kQueryOriginMax;
  ok = ok && kQueryTmin < ray[kQrTmax];
  ok = ok && 0.0f <= ray[kQrTime] && ray[kQrTime] <= 1.0f;  // (-0 passes as 0 does)
  return ok;
}

}  // namespace rt2

#endif  // RT2_QUERY_H_
