// temporal.h — temporal reuse: the image history reprojected across a camera move and blended with the
// current estimate (DESIGN.md §6f, rt2.h "Temporal reuse"), callable from host and device: the GPU kernels
// (temporal.hip), the CPU test program (tests/cpp/temporal_host.cpp) and the numpy statement
// (tests/temporal_ref.py) are this arithmetic.
//
// Float32 throughout; only + - * /, floorf, comparisons and selects, every operation rounded on its own (the
// build's -ffp-contract=off: no fused multiply-add), division correctly rounded, so the three statements agree
// bit for bit. dot(a, b) = (a0 * b0 + a1 * b1) + a2 * b2, cross(a, b) = (a1 * b2 - a2 * b1, a2 * b0 - a0 * b2,
// a0 * b1 - a1 * b0), finite(x) is x - x == 0, min(a, b) = a < b ? a : b, |x| = x < 0 ? 0 - x : x.
//
// Per pixel p of a W x H image (rows bottom-up): the current colour c, variance of the mean v, length n (the
// frames the estimate rests on, n >= 0) and from the 16-float feature record F (rt2.h) the hit flag, the point
// P, the normal nrm, the material index mat (slot 9), the albedo alb and dist. The history is an image of the
// same size: colour ch, variance of the mean vh, length nh (0: none) and the record F' it was taken with, and
// the camera words K' (rt2_camera_params) it was taken under, of which pixel00', du', dv', center' are read.
// The material table (8 floats per material as rt2_scene_materials returns it, or absent) gives the current
// hit's type: 0 (metal) and 2 (dielectric) are specular; a missing table, or an index that is not a whole
// number inside it, counts as diffuse.
//
//   projection   r = P - center', e = pixel00' - center', m = cross(du', dv'), dr = dot(r, m), de = dot(e, m).
//                No history unless dr and de are finite, non-zero and of one sign (P in front of the old
//                camera). s = de / dr, q = r * s - e, fx = dot(q, du') / dot(du', du'),
//                fy = dot(q, dv') / dot(dv', dv'). No history unless fx, fy are finite, -1 <= fx < W and
//                -1 <= fy < H (float comparisons, before any conversion to an integer).
//                x0 = floorf(fx), tx = fx - x0, y0 = floorf(fy), ty = fy - y0.
//   taps         the old pixels (x0 + i, y0 + j), j-major then i, both ascending, with the bilinear weight
//                b = (i ? tx : 1 - tx) * (j ? ty : 1 - ty). A tap is skipped unless it lies inside the image
//                (decided on the integer coordinates: no index is formed for a tap outside), b > 0, nh_q > 0,
//                ch_q and vh_q are finite, the old record is a hit, mat'_q == mat,
//                dot(nrm, nrm'_q) >= min_normal_dot, |dot(nrm, P'_q - P)| <= sigma_p * dist, and the squared
//                distance of the two albedos is <= sigma_a * sigma_a.
//   sums         over the accepted taps, in order: sw = sw + b, sc = sc + b * ch_q, sv = sv + b * vh_q,
//                sn = sn + b * nh_q. The variance is summed with b, not b * b: the bilinear taps of a
//                reprojected image are correlated (neighbouring pixels of the next frame read the same old
//                pixels), so the interpolation is not credited with any averaging. The conservative choice.
//   history      exists iff p is a hit, c and v are finite, sw > 0 and N > 0, N = min(sn / sw, cap), cap =
//                max_history_specular for a specular current hit, else max_history.
//   blend        hc = sc / sw, hv = sv / sw, a = n / (N + n), c' = hc + a * (c - hc) per channel,
//                v' = ((1 - a) * (1 - a)) * hv + (a * a) * v, n' = N + n.
//   no history   c' = c, v' = v, n' = n, bit for bit.
//   not finite   c or v not finite: c' = c, v' = v, n' = 0, so the pixel can never become history.
//
// Degenerate cases, each defined so that no NaN arises from finite inputs (magnitudes up to 2^60 as in
// denoise.h; n >= 0):
//   - dr == 0 (P in the old camera's plane through its centre) or de == 0 (a degenerate camera): no history.
//   - dot(du', du') == 0 or dot(dv', dv') == 0: fx or fy is not finite: no history.
//   - tx == 0 (or ty == 0): the taps with i = 1 (j = 1) have b = 0 and are skipped, whatever they hold.
//   - a 1 x 1 image: fx, fy in [-1, 1): at most the one tap (0, 0) is inside.
//   - dist == 0 (or sigma_p * dist underflowing to 0): the tolerance is 0, only a tap exactly in P's plane
//     passes; no division takes part.
//   - a cap of 0: N = 0, no history (the default for specular hits).
//   - a product or sum that overflows: a comparison with NaN is false, so the tap is skipped.
//   - N > 0 and n >= 0 make N + n > 0: a is in [0, 1].
#ifndef RT2_TEMPORAL_H_
#define RT2_TEMPORAL_H_

#include <cmath>
#include <cstdint>
#include <cstring>

#include "denoise.h"

namespace rt2 {

constexpr int kTemporalCameraWords = 21;   // rt2_camera_params
constexpr int kTemporalMaterialFloats = 8; // rt2_scene_materials

struct TemporalParams {  // rt2_temporal_params
  float max_history, max_history_specular, min_normal_dot, sigma_p, sigma_a;
};

RT2_DN_HD TemporalParams TemporalDefaults() { return TemporalParams{1024.0f, 0.0f, 0.9f, 0.01f, 0.1f}; }

RT2_DN_HD bool TemporalParamsValid(const TemporalParams& k) {
  return DenoiseIsFinite(k.max_history) && k.max_history > 0.0f && DenoiseIsFinite(k.max_history_specular) &&
         k.max_history_specular >= 0.0f && DenoiseIsFinite(k.min_normal_dot) && DenoiseIsFinite(k.sigma_p) &&
         k.sigma_p > 0.0f && DenoiseIsFinite(k.sigma_a) && k.sigma_a > 0.0f;
}

// The history camera: the four vectors read of the 21 words.
struct TemporalCamera {
  float pixel00[3], du[3], dv[3], center[3];
};
RT2_DN_HD TemporalCamera TemporalCameraOf(const float* k) {
  return TemporalCamera{{k[0], k[1], k[2]}, {k[3], k[4], k[5]}, {k[6], k[7], k[8]}, {k[9], k[10], k[11]}};
}

// A history pixel as a tap reads it, four 16-byte words: (ch, vh) (nrm', nh) (P', hit') (alb', mat').
// DenoisePixel's words with the length in dist's place and the material index in the pad's.
struct TemporalPixel {
  float c[3], v;
  float n[3], len;
  float p[3], hit;
  float a[3], mat;
};

// The current pixel's part of its feature record.
struct TemporalCurrent {
  float hit, p[3], n[3], mat, a[3], dist;
};
RT2_DN_HD TemporalCurrent TemporalCurrentOf(const float* f) {
  return TemporalCurrent{f[0], {f[2], f[3], f[4]}, {f[5], f[6], f[7]}, f[9], {f[10], f[11], f[12]}, f[13]};
}
RT2_DN_HD TemporalPixel TemporalPack(const float c[3], float v, float len, const float* f) {
  return TemporalPixel{{c[0], c[1], c[2]}, v, {f[5], f[6], f[7]}, len, {f[2], f[3], f[4]}, f[0], {f[10], f[11], f[12]}, f[9]};
}

RT2_DN_HD float TemporalDot(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// The current hit's cap: materials may be null (every material diffuse). type_bits: word 0 of a material
// holds the type as an integer's bits (the tracer's device table), else as a float (rt2_scene_materials).
RT2_DN_HD float TemporalCap(float mat, const float* materials, int n_materials, bool type_bits, const TemporalParams& k) {
  if (!materials || !(mat >= 0.0f) || !(mat < (float)n_materials)) return k.max_history;
  const int i = (int)mat;
  if ((float)i != mat) return k.max_history;
  const float* m = materials + (size_t)kTemporalMaterialFloats * (size_t)i;
  bool specular = m[0] == 0.0f || m[0] == 2.0f;
  if (type_bits) {
    uint32_t u;
    memcpy(&u, &m[0], sizeof(u));
    specular = u == 0u || u == 2u;
  }
  return specular ? k.max_history_specular : k.max_history;
}

// P's place in the history image. False: no history.
RT2_DN_HD bool TemporalProject(const float P[3], const TemporalCamera& K, int width, int height, float& fx, float& fy) {
  const float r[3] = {P[0] - K.center[0], P[1] - K.center[1], P[2] - K.center[2]};
  const float e[3] = {K.pixel00[0] - K.center[0], K.pixel00[1] - K.center[1], K.pixel00[2] - K.center[2]};
  const float m[3] = {K.du[1] * K.dv[2] - K.du[2] * K.dv[1], K.du[2] * K.dv[0] - K.du[0] * K.dv[2],
                      K.du[0] * K.dv[1] - K.du[1] * K.dv[0]};
  const float dr = TemporalDot(r, m), de = TemporalDot(e, m);
  if (!DenoiseIsFinite(dr) || !DenoiseIsFinite(de) || dr == 0.0f || de == 0.0f || (dr > 0.0f) != (de > 0.0f)) return false;
  const float s = de / dr;
  const float q[3] = {r[0] * s - e[0], r[1] * s - e[1], r[2] * s - e[2]};
  fx = TemporalDot(q, K.du) / TemporalDot(K.du, K.du);
  fy = TemporalDot(q, K.dv) / TemporalDot(K.dv, K.dv);
  if (!DenoiseIsFinite(fx) || !DenoiseIsFinite(fy)) return false;
  return fx >= -1.0f && fx < (float)width && fy >= -1.0f && fy < (float)height;
}

struct TemporalSums {
  float sc[3], sv, sn, sw;
};

// One tap inside the image with bilinear weight b.
RT2_DN_HD void TemporalTap(TemporalSums& s, const TemporalCurrent& p, const TemporalPixel& q, float b, const TemporalParams& k) {
  if (!(b > 0.0f) || !(q.len > 0.0f) || !DenoisePixelFinite(q.c, q.v) || q.hit == 0.0f || !(q.mat == p.mat)) return;
  if (!(TemporalDot(p.n, q.n) >= k.min_normal_dot)) return;
  const float d[3] = {q.p[0] - p.p[0], q.p[1] - p.p[1], q.p[2] - p.p[2]};
  if (!(DenoiseAbs(TemporalDot(p.n, d)) <= k.sigma_p * p.dist)) return;
  const float da[3] = {q.a[0] - p.a[0], q.a[1] - p.a[1], q.a[2] - p.a[2]};
  if (!(TemporalDot(da, da) <= k.sigma_a * k.sigma_a)) return;
  s.sw = s.sw + b;
  s.sc[0] = s.sc[0] + b * q.c[0];
  s.sc[1] = s.sc[1] + b * q.c[1];
  s.sc[2] = s.sc[2] + b * q.c[2];
  s.sv = s.sv + b * q.v;
  s.sn = s.sn + b * q.len;
}

struct TemporalResult {
  float c[3], v, len;
};

// The whole pixel. fetch(x, y) returns the history's TemporalPixel at a pixel inside the image.
template <class Fetch>
RT2_DN_HD TemporalResult TemporalResolvePixel(const float c[3], float v, float len, const float* features,
                                              const TemporalCamera& K, int width, int height, const float* materials,
                                              int n_materials, bool type_bits, const TemporalParams& k, Fetch fetch) {
  TemporalResult o{{c[0], c[1], c[2]}, v, len};
  if (!DenoisePixelFinite(c, v)) {
    o.len = 0.0f;
    return o;
  }
  const TemporalCurrent p = TemporalCurrentOf(features);
  if (p.hit == 0.0f) return o;
  float fx, fy;
  if (!TemporalProject(p.p, K, width, height, fx, fy)) return o;
  const float fx0 = floorf(fx), fy0 = floorf(fy);
  const float tx = fx - fx0, ty = fy - fy0;
  const int x0 = (int)fx0, y0 = (int)fy0;  // in [-1, width - 1] x [-1, height - 1]
  TemporalSums s{{0.0f, 0.0f, 0.0f}, 0.0f, 0.0f, 0.0f};
  for (int j = 0; j < 2; j++) {
    for (int i = 0; i < 2; i++) {
      const int x = x0 + i, y = y0 + j;
      if (x < 0 || x >= width || y < 0 || y >= height) continue;
      const float b = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
      if (!(b > 0.0f)) continue;
      TemporalTap(s, p, fetch(x, y), b, k);
    }
  }
  if (!(s.sw > 0.0f)) return o;
  const float cap = TemporalCap(p.mat, materials, n_materials, type_bits, k);
  const float mean_n = s.sn / s.sw;
  const float N = mean_n < cap ? mean_n : cap;
  if (!(N > 0.0f)) return o;
  const float a = len / (N + len);
  const float ia = 1.0f - a;
  for (int ch = 0; ch < 3; ch++) {
    const float hc = s.sc[ch] / s.sw;
    o.c[ch] = hc + a * (c[ch] - hc);
  }
  const float hv = s.sv / s.sw;
  o.v = (ia * ia) * hv + (a * a) * v;
  o.len = N + len;
  return o;
}

}  // namespace rt2

#endif  // RT2_TEMPORAL_H_
