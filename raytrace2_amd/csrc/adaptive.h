// adaptive.h — the per-pixel rules of adaptive sampling (rt2.h "Adaptive sampling"), callable from host and
// device: the GPU kernels (adaptive.hip) and the CPU test program (tests/cpp/adaptive_host.cpp) run these
// functions.
//
// A pixel with sample count n_p >= 2 and float32 sums a (samples) and q (squares) over its n_p frames is
// `over` unless its noise estimate is finite and at most the threshold:
//   over = !(finite && err <= (double)threshold),   err = NoiseOfPixel(a, q, n_p).err   (noise.h)
// so a pixel with a non-finite sum is always over. An active pixel at column x of a row stays active iff
// some pixel of the same row in the columns [x - window, x + window] within [0, width) is over; otherwise
// it retires. The window runs along the row only: a partition holds whole rows, so the decision needs no
// other GPU's pixels and does not depend on the partition.
#ifndef RT2_ADAPTIVE_H_
#define RT2_ADAPTIVE_H_

#include <cstdint>

#include "noise.h"

namespace rt2 {

constexpr int kAdaptiveWindowMax = 64;  // 0 <= window <= 64

struct PixelOver {
  bool over;
  bool finite;
};

RT2_NOISE_HD PixelOver AdaptiveOver(const float a[3], const float q[3], uint32_t n, double threshold) {
  const PixelNoise p = NoiseOfPixel(a, q, (int64_t)n);
  PixelOver o;
  o.finite = p.finite;
  o.over = !(p.finite && p.err <= threshold);
  return o;
}

// over: the `over` flags (0 / 1) of the columns [base, ...) of one row, holding at least the columns
// [max(x - window, 0), min(x + window, width - 1)]. True iff one of those columns is over.
RT2_NOISE_HD bool AdaptiveWindowOver(const uint8_t* over, int base, int x, int width, int window) {
  const int lo = x - window > 0 ? x - window : 0;
  const int hi = x + window < width - 1 ? x + window : width - 1;
  for (int c = lo; c <= hi; c++)
    if (over[c - base]) return true;
  return false;
}

// One classify workgroup's share of the check's scalars (256 pixels).
struct AdaptivePartial {
  uint64_t nonfinite;  // pixels with a non-finite sum
  uint64_t samples;    // sum of n_p
};

// rt2_adaptive's additive fields as the scan kernel leaves them on the device.
struct AdaptiveTotals {
  uint64_t active, retired, nonfinite, samples;
};

}  // namespace rt2

#endif  // RT2_ADAPTIVE_H_
