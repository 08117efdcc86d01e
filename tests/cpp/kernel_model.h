// The kernel's lane semantics on the host, once: what the proof harnesses of tests/cpp walk and compare
// (render.hip trace_linear and the functions it calls: the same step semantics, operation order and roundings;
// build with -ffp-contract=off). A change to a step's semantics is made here, and every harness sees it.
//   bits and math    B, F, Ulps, HostMath (the host restatement of render.hip BoxMath), kAbove1e8, kTmin, V3
//   primitive tests  AabbHit, QuadAA, QuadCand
//   transform entry  XformEntry
//   the walk         Walk over lin_wide or flat_wide, the flat certificate evaluated eagerly or lazily
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scene.h"
#ifndef RT2_BOXAA_FN
#define RT2_BOXAA_FN inline
#endif
#include "boxaa.h"

namespace kernel_model {
using namespace rt2;

inline uint32_t B(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}
inline float F(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}
inline float Ulps(float x, int n) {  // x moved by n ulps
  if (x == 0.0f) return n == 0 ? x : std::ldexp((float)n, -149);
  uint32_t b = B(x);
  if ((x > 0) == (n > 0)) b += (uint32_t)std::abs(n); else b -= (uint32_t)std::abs(n);
  return F(b);
}
struct HostMath {
  static float div(float a, float b, float inv) {
    const float q = a * inv;
    return std::fma(std::fma(-b, q, a), inv, q);
  }
  static float min(float a, float b) { return std::fmin(a, b); }
  static float max(float a, float b) { return std::fmax(a, b); }
  static float min3(float a, float b, float c) { return std::fmin(std::fmin(a, b), c); }
  static float max3(float a, float b, float c) { return std::fmax(std::fmax(a, b), c); }
  static float amin3(float a, float b, float c) { return min3(std::fabs(a), std::fabs(b), std::fabs(c)); }
  static float amax3(float a, float b, float c) { return max3(std::fabs(a), std::fabs(b), std::fabs(c)); }
  static float med3(float a, float b, float c) { return std::fmax(std::fmin(a, b), std::fmin(std::fmax(a, b), c)); }
  static float fma(float a, float b, float c) { return std::fma(a, b, c); }
  static float abs(float a) { return std::fabs(a); }
  static uint32_t bits(float a) { return B(a); }
};
constexpr float kAbove1e8 = 0x1.5798f0p-27f;
constexpr float kTmin = 0.001f;

struct V3 {
  float x, y, z;
  float operator[](int k) const { return k == 0 ? x : (k == 1 ? y : z); }
};
inline float Dot(V3 a, V3 b) {
  const float px = a.x * b.x, py = a.y * b.y, pz = a.z * b.z;
  return (px + py) + pz;
}
inline V3 Cross(V3 a, V3 b) { return V3{a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
inline bool Finite3(V3 v) { return std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z); }
inline float Gmax(float x, float y) { return (x < y) ? y : x; }
inline float Gmin(float x, float y) { return (y < x) ? y : x; }

// render.hip aabb_hit (AABB::Hit, AABB.hpp:34-47), for rays whose reciprocal is not finite
inline bool AabbHit(const float* lo, const float* hi, V3 o, V3 inv, float tmin, float tmax) {
  for (int k = 0; k < 3; k++) {
    float t0 = (lo[k] - o[k]) * inv[k], t1 = (hi[k] - o[k]) * inv[k];
    if (t1 < t0) std::swap(t0, t1);
    tmin = Gmax(t0, tmin);
    tmax = Gmin(t1, tmax);
    if (tmax <= tmin) return false;
  }
  return true;
}

// render.hip quad_aa<K>: the rejection word of a QUADAA record
inline uint32_t QuadAA(int k, const float* r, V3 o, V3 d, V3 inv, float& t_out) {
  const int a = (k + 1) % 3, b = (k + 2) % 3;
  const float dk = d[k];
  const float t = HostMath::div(r[0] - o[k], dk, inv[k]);
  const float pa = o[a] + d[a] * t, pb = o[b] + d[b] * t;
  t_out = t;
  return (B(pa - r[1]) | B(r[2] - pa) | B(pb - r[3])) | (B(r[4] - pb) | B(std::fabs(dk) - kAbove1e8));
}
// render.hip quad_cand_u on a QUAD record's 20 words, axis codes 0..3 (4..6 with the QUAD layout do not
// occur: the compiler gives such quads code K + 1)
inline bool QuadCand(uint32_t axis, const float* w, V3 o, V3 d, float& t_out) {
  if (axis >= 1 && axis <= 3) {
    const int k = (int)axis - 1, a = (k + 1) % 3, b = (k + 2) % 3;
    const float nk = w[k], wk = w[16 + k];
    const float n_dot = nk * d[k];
    const float t = (w[3] - nk * o[k]) / n_dot;
    const float pva = (o[a] + d[a] * t) - w[4 + a];
    const float pvb = (o[b] + d[b] * t) - w[4 + b];
    const float alpha = wk * (pva * w[12 + b] - w[12 + a] * pvb);
    const float beta = wk * (w[8 + a] * pvb - pva * w[8 + b]);
    t_out = t;
    return !(std::fabs(n_dot) <= 1e-8f) && (0.0f <= alpha && alpha <= 1.0f) && (0.0f <= beta && beta <= 1.0f);
  }
  const V3 n{w[0], w[1], w[2]};
  const float n_dot = Dot(n, d);
  const float t = (w[3] - Dot(n, o)) / n_dot;
  const V3 p{o.x + d.x * t, o.y + d.y * t, o.z + d.z * t};
  const V3 pv{p.x - w[4], p.y - w[5], p.z - w[6]};
  const V3 ww{w[16], w[17], w[18]};
  const float alpha = Dot(ww, Cross(pv, V3{w[12], w[13], w[14]}));
  const float beta = Dot(ww, Cross(V3{w[8], w[9], w[10]}, pv));
  t_out = t;
  return !(std::fabs(n_dot) <= 1e-8f) && (0.0f <= alpha && alpha <= 1.0f) && (0.0f <= beta && beta <= 1.0f);
}

// A kXform step's entry on the transform's record m: the ray into model space (the y-axis form or the general
// one), the direction normalised, its reciprocal.
inline void XformEntry(const float* m, V3& o, V3& d, V3& inv) {
  V3 no, nd;
  if (B(m[11]) == kXformYAxis) {
    no = V3{m[0] * o.x + (m[8] * o.z + m[12]), m[5] * o.y + m[13], m[2] * o.x + (m[10] * o.z + m[14])};
    nd = V3{m[0] * d.x + m[8] * d.z, m[5] * d.y, m[2] * d.x + m[10] * d.z};
  } else {
    no = V3{(m[0] * o.x + m[4] * o.y) + (m[8] * o.z + m[12]), (m[1] * o.x + m[5] * o.y) + (m[9] * o.z + m[13]),
            (m[2] * o.x + m[6] * o.y) + (m[10] * o.z + m[14])};
    nd = V3{m[0] * d.x + m[4] * d.y + m[8] * d.z, m[1] * d.x + m[5] * d.y + m[9] * d.z,
            m[2] * d.x + m[6] * d.y + m[10] * d.z};
  }
  o = no;
  const float s = 1.0f / std::sqrt(Dot(nd, nd));  // (rcp_nr(sqrt_nr(.)) is this, bit for bit, in its range)
  d = V3{nd.x * s, nd.y * s, nd.z * s};
  inv = V3{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
}

struct Result {
  uint32_t prim = kRefNone;
  float t = FLT_MAX;
  bool uncert = false;  // flat walk only
  bool xform = false;   // flat walk only: the winner's row of the certificate table carries kFlatCertXform
  bool wfin = false;    // the world ray's reciprocal is finite
};

enum Program { kLinWide, kFlatWide };  // the BVH program (slab test per node, skip on a miss) or the flat one
// How a flat walk evaluates its certificate. kEager restates the earlier evaluation: FlatCertRule at every kXform
// step on the step's own box with the lane's tmax there (xfail), carried to the exit when the closest hit lies
// under the transform (xunc), and the end rule on the winner's row with T = its t, of which one verdict is read
// by the row's flag. kLazy is the kernel's: t_entry kept at the kXform step, t_keep = t_entry at such an exit, and
// one rule after the walk on the winner's row with T = flag ? t_keep : t.
enum Cert { kEager, kLazy };
struct WalkOptions {
  Program program;
  Cert cert;      // (read by a flat walk only)
  uint32_t mode;  // the launch's FlatMode
};

// One lane's trace of a wide program (render.hip trace_linear). Returns false for a step the model does not hold.
inline bool Walk(const CompiledScene& c, const WalkOptions& opt, V3 wo, V3 wd, Result& out) {
  const bool flat = opt.program == kFlatWide;
  const std::vector<uint32_t>& prog = flat ? c.flat_wide : c.lin_wide;
  const float* recs = c.lind.data();
  V3 o = wo, d = wd;
  V3 inv{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
  const V3 winv = inv;
  bool fin = Finite3(inv);
  const bool wfin = fin;
  float tmax = FLT_MAX;
  uint32_t prim = kRefNone;
  bool xfail = false, xunc = false;           // kEager
  float t_entry = FLT_MAX, t_keep = FLT_MAX;  // kLazy
  uint32_t i = 0;
  for (size_t guard = 0; guard < 100000; guard++) {
    const uint32_t* sw = &prog[16 * (size_t)i];
    const uint32_t kind = sw[0], off = sw[2];
    if (kind == kProgramEnd) break;
    if (kind == kBvh) {
      if (flat || sw[2] != i + 1u) return false;  // (no BVH step in a flat program; no paired steps without spheres)
      const float lo[3] = {F(sw[4]), F(sw[5]), F(sw[6])}, hi[3] = {F(sw[8]), F(sw[9]), F(sw[10])};
      // (the kernel takes aabb_hit_fin when the whole wave's reciprocals are finite and aabb_hit otherwise: equal
      // for a lane with a finite reciprocal, rt2_selftest which 1)
      const bool in = fin ? FlatCertRule<HostMath>(lo, hi, o.x, o.y, o.z, inv.x, inv.y, inv.z, kTmin, tmax)
                          : AabbHit(lo, hi, o, inv, kTmin, tmax);
      i = in ? i + 1u : sw[1];
    } else if (kind == kQuad) {
      const uint32_t run = sw[3] & kRunLenMask;
      bool boxed = false;
      if ((int32_t)sw[3] < 0) {
        const float* bw = recs + 4 * (size_t)(off - (uint32_t)kBoxAARecords);
        const uint32_t kmax0 = B(tmax) - B(kTmin);
        const BoxAAResult r = BoxAATest<HostMath>(bw, bw[6], o.x, o.y, o.z, d.x, d.y, d.z, inv.x, inv.y, inv.z, kTmin);
        if (r.cert) {
          if (r.x <= kmax0) {
            tmax = r.t;
            prim = make_ref(kQuadAA, off + r.face * (uint32_t)kQuadRecords);
          }
          boxed = true;
        }
      }
      if (!boxed) {
        uint32_t codes = sw[1], kmax = B(tmax) - B(kTmin), vref = make_ref(kQuadAA, off);
        const float* r = recs + 4 * (size_t)off;
        while (true) {
          const uint32_t c0 = codes & 7u;
          float t0;
          if (c0 >= 4u) {
            const uint32_t rej = QuadAA((int)c0 - 4, r, o, d, inv, t0);
            const uint32_t x = (B(t0) - B(kTmin)) | (rej & 0x80000000u);
            if (x <= kmax) prim = vref;
            kmax = std::min(kmax, x);
          } else {
            const bool ok0 = QuadCand(c0, r, o, d, t0);
            const uint32_t kt = B(t0) - B(kTmin);
            if (ok0 && kt <= kmax) {
              kmax = kt;
              prim = vref ^ ((kQuadAA ^ kQuad) << 28);
            }
          }
          codes >>= 3;
          if (codes == 1u) break;
          r += 4 * kQuadRecords;
          vref += (uint32_t)kQuadRecords;
        }
        tmax = F(kmax + B(kTmin));
      }
      i += run;
    } else if (kind == kXform) {
      if (flat && opt.cert == kEager) {
        // the entry rule on the step's own box with the ray the lane carries here (the world ray: flat
        // programs nest no transform) and T = the lane's tmax here
        const float lo[3] = {F(sw[4]), F(sw[5]), F(sw[6])}, hi[3] = {F(sw[7]), F(sw[8]), F(sw[9])};
        xfail = !FlatCertRule<HostMath>(lo, hi, o.x, o.y, o.z, inv.x, inv.y, inv.z, kTmin, tmax);
      } else {
        t_entry = tmax;
      }
      XformEntry(recs + 4 * (size_t)off, o, d, inv);
      fin = Finite3(inv);
      i++;
    } else if (kind == kXformExit) {
      if (sw[3] != kRefNone) return false;  // (flat programs and their BVH programs nest no transform)
      if (prim - make_ref(prim >> 28, off + (uint32_t)kXformRecords) < sw[1] - (off + (uint32_t)kXformRecords)) {
        if (opt.cert == kEager) xunc = xfail; else t_keep = t_entry;
      }
      o = wo;
      d = wd;
      inv = winv;
      fin = wfin;
      i++;
    } else {
      return false;
    }
  }
  out.prim = prim;
  out.t = tmax;
  out.uncert = false;
  out.xform = false;
  out.wfin = wfin;
  if (flat && prim != kRefNone) {
    const float* ct = &c.flat_cert[4 * (size_t)(prim & kOffsetMask)];
    out.xform = B(ct[3]) == kFlatCertXform;
    if (opt.cert == kEager) {
      const bool end_ok = FlatCertRule<HostMath>(ct, ct + 4, wo.x, wo.y, wo.z, winv.x, winv.y, winv.z, kTmin, tmax);
      out.uncert = !wfin || opt.mode == kFlatCertifyNothing || (out.xform ? xunc : !end_ok);
    } else {
      const float T = out.xform ? t_keep : tmax;
      const bool rule = FlatCertRule<HostMath>(ct, ct + 4, wo.x, wo.y, wo.z, winv.x, winv.y, winv.z, kTmin, T);
      out.uncert = !wfin || opt.mode == kFlatCertifyNothing || !rule;
    }
  }
  return true;
}
}  // namespace kernel_model
