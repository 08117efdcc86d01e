// denoise.h — the variance-guided a-trous filter (DESIGN.md §6e, rt2.h "Feature buffers and denoiser"),
// callable from host and device: the GPU kernels (denoise.hip), the CPU test program
// (tests/cpp/denoise_host.cpp) and the numpy statement (tests/denoise_ref.py) are this arithmetic.
//
// Float32 throughout; only + - * /, sqrt, comparisons and selects, every operation rounded on its own (the
// build's -ffp-contract=off: no fused multiply-add), division and square root correctly rounded. The
// edge-stopping functions are rational (1 / (1 + x^2)), so the three statements agree bit for bit.
//
// Per pixel p: colour c_p, variance of the mean v_p, and from the 16-float feature record (rt2.h) the hit
// flag, the point P, the normal n, the albedo a and dist (camera centre to P). A pixel is finite iff c_p
// and v_p are finite. The feature values of a finite pixel must be finite.
//
// Pass i = 0 .. iterations-1 has step s = 1 << i and reads one buffer, writes the other.
//   vbar_p   DenoiseVbar: the pass's variance over the 3x3 neighbourhood at stride 1 (dy then dx ascending),
//            weights 1/4 (centre), 1/8 (edge), 1/16 (corner), over the taps inside the image that are finite
//            and have p's hit flag: sv = sv + w * v_q, sw = sw + w, vbar = sv / sw. The centre always
//            counts, so sw >= 1/4.
//   taps     q = p + s * (dx, dy), dx, dy in -2..2, dy-major then dx, both ascending; a tap outside the image
//            is skipped. h = k[|dx|] * k[|dy|], k = {3/8, 1/4, 1/16} (exact in binary, so is every product).
//   weight   the centre tap: h(0, 0). Another tap is skipped unless q is finite and hit_q == hit_p; else
//              w = h * wl, and when both are hits w = ((w * wn) * wp) * wa                 (DenoiseTapWeight)
//              wl = 1 / (1 + xl * xl), xl = |l_p - l_q| / (sigma_l * sqrt(max(vbar_p, 0)) + eps_l),
//                   l = ((r + g) + b) / 3
//              wn = max(0, dot(n_p, n_q)) squared normal_power_log2 times, dot = (x * x + y * y) + z * z
//              wp = 1 / (1 + xp * xp), xp = |dot(n_p, P_q - P_p)| / (sigma_p * dist_p)
//              wa = 1 / (1 + da / (sigma_a * sigma_a)), da = the squared distance of the two albedos
//   sums     over the taps not skipped, in tap order: sw = sw + w, sc = sc + w * c_q, sv = sv + (w * w) * v_q
//   output   c' = sc / sw, v' = sv / (sw * sw)                                               (DenoiseFinish)
//
// Degenerate cases, each defined so that no NaN arises from finite inputs (magnitudes up to 2^60, far past
// any radiance; beyond that the sums themselves can overflow):
//   - p not finite: its colour and variance pass through unchanged, in every pass.
//   - dist_p == 0 (or sigma_p * dist_p underflowing to 0): wp = 1 (no 0 / 0).
//   - vbar_p == 0 (a flat region): the denominator of xl is eps_l > 0. A negative caller variance counts
//     as 0 under the square root.
//   - l_p - l_q not a number (both luminances overflowed): wl = 0.
//   - no neighbour contributes (every other tap skipped or of weight 0): the centre comes back bit for bit,
//     c' = c_p and v' = v_p (h * c / h need not round back to c).
//   - an x that overflows to +inf gives a weight of 1 / inf = 0.
#ifndef RT2_DENOISE_H_
#define RT2_DENOISE_H_

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RT2_DN_HD __host__ __device__ inline
#else
#define RT2_DN_HD inline
#endif

namespace rt2 {

constexpr int kDenoiseFeatureFloats = 16;  // rt2.h: the feature record
constexpr int kDenoiseIterMax = 8, kDenoiseNormalPowMax = 8;

struct DenoiseParams {  // rt2_denoise_params
  int iterations;
  int normal_power_log2;
  float sigma_l, sigma_p, sigma_a, eps_l;
};

RT2_DN_HD DenoiseParams DenoiseDefaults() { return DenoiseParams{5, 7, 1.0f, 0.01f, 0.1f, 1e-3f}; }

// A pixel as the filter reads it, four 16-byte words: (c, v) (n, dist) (P, hit) (a, 0).
struct DenoisePixel {
  float c[3], v;
  float n[3], dist;
  float p[3], hit;
  float a[3], pad;
};

RT2_DN_HD float DenoiseSqrt(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return sqrtf(x);  // correctly rounded (hipcc's default for float32 division and sqrt)
#else
  return std::sqrt(x);  // IEEE 754: correctly rounded
#endif
}

RT2_DN_HD bool DenoiseIsFinite(float x) { return x - x == 0.0f; }  // false for NaN and +-inf
RT2_DN_HD bool DenoisePixelFinite(const float c[3], float v) {
  return DenoiseIsFinite(c[0]) && DenoiseIsFinite(c[1]) && DenoiseIsFinite(c[2]) && DenoiseIsFinite(v);
}
RT2_DN_HD float DenoiseAbs(float x) { return x < 0.0f ? 0.0f - x : x; }
RT2_DN_HD float DenoiseLuminance(const float c[3]) { return ((c[0] + c[1]) + c[2]) / 3.0f; }
RT2_DN_HD float DenoiseKernel1(int d) {  // k[|d|], |d| <= 2
  const int a = d < 0 ? -d : d;
  return a == 0 ? 0.375f : (a == 1 ? 0.25f : 0.0625f);
}
RT2_DN_HD float DenoiseVbarWeight(int dx, int dy) {
  const int a = (dx != 0 ? 1 : 0) + (dy != 0 ? 1 : 0);
  return a == 0 ? 0.25f : (a == 1 ? 0.125f : 0.0625f);
}

// vbar's running sums: DenoiseVbarTap for each tap of the 3x3 neighbourhood inside the image, in order.
struct DenoiseVbarSums {
  float sv, sw;
};
RT2_DN_HD void DenoiseVbarTap(DenoiseVbarSums& s, float hit_p, const float cq[3], float vq, float hit_q, int dx, int dy) {
  if (!DenoisePixelFinite(cq, vq) || hit_q != hit_p) return;
  const float w = DenoiseVbarWeight(dx, dy);
  s.sv = s.sv + w * vq;
  s.sw = s.sw + w;
}
RT2_DN_HD float DenoiseVbarFinish(const DenoiseVbarSums& s) { return s.sv / s.sw; }

// What a pass needs of its centre pixel once: the luminance and the denominators of xl and xp.
struct DenoiseCentre {
  float l, den_l, den_p;
};
RT2_DN_HD DenoiseCentre DenoiseCentreOf(const DenoisePixel& p, float vbar, const DenoiseParams& k) {
  DenoiseCentre c;
  c.l = DenoiseLuminance(p.c);
  const float vb = vbar > 0.0f ? vbar : 0.0f;
  c.den_l = k.sigma_l * DenoiseSqrt(vb) + k.eps_l;
  c.den_p = k.sigma_p * p.dist;
  return c;
}

// The weight of tap q != p with kernel weight h; q is finite and has p's hit flag (the caller skipped
// the others).
RT2_DN_HD float DenoiseTapWeight(const DenoisePixel& p, const DenoiseCentre& pc, const DenoisePixel& q, float h,
                                 const DenoiseParams& k) {
  const float dl = pc.l - DenoiseLuminance(q.c);
  const float xl = DenoiseAbs(dl) / pc.den_l;
  float wl = 1.0f / (1.0f + xl * xl);
  if (!(dl == dl)) wl = 0.0f;
  float w = h * wl;
  if (p.hit != 0.0f) {
    float wn = (p.n[0] * q.n[0] + p.n[1] * q.n[1]) + p.n[2] * q.n[2];
    wn = wn > 0.0f ? wn : 0.0f;
    for (int i = 0; i < k.normal_power_log2; i++) wn = wn * wn;
    const float d0 = q.p[0] - p.p[0], d1 = q.p[1] - p.p[1], d2 = q.p[2] - p.p[2];
    const float pd = (p.n[0] * d0 + p.n[1] * d1) + p.n[2] * d2;
    float wp = 1.0f;
    if (pc.den_p > 0.0f) {
      const float xp = DenoiseAbs(pd) / pc.den_p;
      wp = 1.0f / (1.0f + xp * xp);
    }
    const float a0 = q.a[0] - p.a[0], a1 = q.a[1] - p.a[1], a2 = q.a[2] - p.a[2];
    const float da = (a0 * a0 + a1 * a1) + a2 * a2;
    const float wa = 1.0f / (1.0f + da / (k.sigma_a * k.sigma_a));
    w = ((w * wn) * wp) * wa;
  }
  return w;
}

// A pixel's running sums over its taps, in tap order.
struct DenoiseSums {
  float sc[3], sv, sw;
  bool any;  // a tap other than the centre had a weight > 0
};
RT2_DN_HD DenoiseSums DenoiseSumsZero() { return DenoiseSums{{0.0f, 0.0f, 0.0f}, 0.0f, 0.0f, false}; }
RT2_DN_HD void DenoiseAdd(DenoiseSums& s, float w, const float cq[3], float vq) {
  s.sw = s.sw + w;
  s.sc[0] = s.sc[0] + w * cq[0];
  s.sc[1] = s.sc[1] + w * cq[1];
  s.sc[2] = s.sc[2] + w * cq[2];
  s.sv = s.sv + (w * w) * vq;
}
// One tap of finite pixel p (dx, dy in -2..2; q the pixel there, inside the image).
RT2_DN_HD void DenoiseTap(DenoiseSums& s, const DenoisePixel& p, const DenoiseCentre& pc, const DenoisePixel& q, int dx,
                          int dy, const DenoiseParams& k) {
  const float h = DenoiseKernel1(dx) * DenoiseKernel1(dy);
  if (dx == 0 && dy == 0) {
    DenoiseAdd(s, h, p.c, p.v);
    return;
  }
  if (!DenoisePixelFinite(q.c, q.v) || q.hit != p.hit) return;
  const float w = DenoiseTapWeight(p, pc, q, h, k);
  s.any = s.any || w > 0.0f;
  DenoiseAdd(s, w, q.c, q.v);
}
RT2_DN_HD void DenoiseFinish(const DenoiseSums& s, const DenoisePixel& p, float out_c[3], float& out_v) {
  if (!s.any) {
    out_c[0] = p.c[0], out_c[1] = p.c[1], out_c[2] = p.c[2];
    out_v = p.v;
    return;
  }
  out_c[0] = s.sc[0] / s.sw;
  out_c[1] = s.sc[1] / s.sw;
  out_c[2] = s.sc[2] / s.sw;
  out_v = s.sv / (s.sw * s.sw);
}

// The 16-float feature record -> the filter's three feature words of a pixel.
RT2_DN_HD void DenoiseUnpackFeatures(const float* f, DenoisePixel& o) {
  o.hit = f[0];
  o.p[0] = f[2], o.p[1] = f[3], o.p[2] = f[4];
  o.n[0] = f[5], o.n[1] = f[6], o.n[2] = f[7];
  o.a[0] = f[10], o.a[1] = f[11], o.a[2] = f[12];
  o.dist = f[13];
  o.pad = 0.0f;
}

// The tracer path's variance of the mean from the float3 standard error (rt2_tracer_standard_error).
RT2_DN_HD float DenoiseVarianceOfSem(const float sem[3]) {
  return ((sem[0] * sem[0] + sem[1] * sem[1]) + sem[2] * sem[2]) / 3.0f;
}

RT2_DN_HD bool DenoiseParamsValid(const DenoiseParams& k) {
  const bool ints = k.iterations >= 1 && k.iterations <= kDenoiseIterMax && k.normal_power_log2 >= 0 &&
                    k.normal_power_log2 <= kDenoiseNormalPowMax;
  const bool f = DenoiseIsFinite(k.sigma_l) && k.sigma_l > 0.0f && DenoiseIsFinite(k.sigma_p) && k.sigma_p > 0.0f &&
                 DenoiseIsFinite(k.sigma_a) && k.sigma_a > 0.0f && DenoiseIsFinite(k.eps_l) && k.eps_l > 0.0f;
  return ints && f;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The whole filter on the host over packed pixels px[h][w] (tests/cpp/denoise_host.cpp): the passes'
// colour and variance ping-pong between px and a scratch copy; the result is left in px.
inline void DenoiseHost(DenoisePixel* px, DenoisePixel* scratch, int w, int h, const DenoiseParams& k) {
  DenoisePixel* src = px;
  DenoisePixel* dst = scratch;
  for (long i = 0; i < (long)w * h; i++) scratch[i] = px[i];
  for (int it = 0; it < k.iterations; it++) {
    const int s = 1 << it;
    for (int y = 0; y < h; y++) {
      for (int x = 0; x < w; x++) {
        const DenoisePixel& p = src[(long)y * w + x];
        DenoisePixel& o = dst[(long)y * w + x];
        if (!DenoisePixelFinite(p.c, p.v)) {
          o.c[0] = p.c[0], o.c[1] = p.c[1], o.c[2] = p.c[2], o.v = p.v;
          continue;
        }
        DenoiseVbarSums vs{0.0f, 0.0f};
        for (int dy = -1; dy <= 1; dy++)
          for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
            const DenoisePixel& q = src[(long)qy * w + qx];
            DenoiseVbarTap(vs, p.hit, q.c, q.v, q.hit, dx, dy);
          }
        const DenoiseCentre pc = DenoiseCentreOf(p, DenoiseVbarFinish(vs), k);
        DenoiseSums sm = DenoiseSumsZero();
        for (int dy = -2; dy <= 2; dy++)
          for (int dx = -2; dx <= 2; dx++) {
            const long qx = (long)x + (long)s * dx, qy = (long)y + (long)s * dy;
            if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
            DenoiseTap(sm, p, pc, src[qy * w + qx], dx, dy, k);
          }
        DenoiseFinish(sm, p, o.c, o.v);
      }
    }
    DenoisePixel* t = src;
    src = dst;
    dst = t;
  }
  if (src != px)
    for (long i = 0; i < (long)w * h; i++) px[i] = src[i];
}
#endif

}  // namespace rt2

#endif  // RT2_DENOISE_H_
