// noise.h — the per-pixel noise estimate (DESIGN.md "Noise estimate"), callable from host and device:
// the GPU kernel (noise.hip) and the CPU test program (tests/cpp/noise_host.cpp) run this one function.
//
// Inputs: n >= 2 frames accumulated, and a pixel's float32 sums over those frames in frame order, a_c of
// the samples (the accumulation) and q_c of their squares (moment2). All arithmetic is in double, every
// operation rounded on its own (the build's -ffp-contract=off: no fused multiply-add), the square roots
// correctly rounded:
//   mean_c = a_c / n
//   ss_c   = q_c - a_c * mean_c, clamped to 0 unless > 0 (rounding can push it below 0)
//   sem_c  = (float) sqrt(ss_c / ((double)n * (n - 1)))              standard error of the mean
//   err    = sqrt((sem_r^2 + sem_g^2 + sem_b^2) / 3) / max(1, (mean_r + mean_g + mean_b) / 3)
// err uses the float32-rounded sem_c; its divisor discounts pixels the display clamps anyway (ToColor
// clamps to [0, 1]). A pixel with a non-finite a_c or q_c has sem = err = +inf and finite = false.
#ifndef RT2_NOISE_H_
#define RT2_NOISE_H_

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RT2_NOISE_HD __host__ __device__ inline
#else
#define RT2_NOISE_HD inline
#endif

namespace rt2 {

struct PixelNoise {
  float sem[3];
  double err;
  bool finite;
};

RT2_NOISE_HD double NoiseSqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsqrt_rn(x);
#else
  return std::sqrt(x);  // IEEE 754: correctly rounded
#endif
}

RT2_NOISE_HD bool NoiseFinite(float x) { return x - x == 0.0f; }  // false for NaN and +-inf

RT2_NOISE_HD PixelNoise NoiseOfPixel(const float a[3], const float q[3], int64_t n) {
  PixelNoise o;
  o.finite = true;
  for (int c = 0; c < 3; c++) o.finite = o.finite && NoiseFinite(a[c]) && NoiseFinite(q[c]);
  if (!o.finite) {
    o.sem[0] = o.sem[1] = o.sem[2] = INFINITY;
    o.err = (double)INFINITY;
    return o;
  }
  const double dn = (double)n;
  const double denom = dn * (double)(n - 1);
  double mean[3], s[3];
  for (int c = 0; c < 3; c++) {
    const double ac = (double)a[c];
    mean[c] = ac / dn;
    const double prod = ac * mean[c];
    double ss = (double)q[c] - prod;
    if (!(ss > 0.0)) ss = 0.0;
    o.sem[c] = (float)NoiseSqrt(ss / denom);
    s[c] = (double)o.sem[c];
  }
  const double v = (s[0] * s[0] + s[1] * s[1] + s[2] * s[2]) / 3.0;
  const double m = (mean[0] + mean[1] + mean[2]) / 3.0;
  o.err = NoiseSqrt(v) / (m > 1.0 ? m : 1.0);
  return o;
}

// One workgroup's share of the image's noise scalars (noise.hip writes one per 256 pixels; the host
// adds them up in block order, so the same image gives the same bits every time).
struct NoisePartial {
  double sum_sq;   // sum of err^2 over the finite pixels
  double max_err;  // largest finite err (0: none)
  uint64_t below;  // pixels with err <= threshold
  uint64_t nonfinite;
};

}  // namespace rt2

#endif  // RT2_NOISE_H_
