// Host proof check of the flat walk's certificate (rt2_layout.h "Flat program", boxaa.h FlatCertRule,
// DESIGN.md §4 "Flat walk of small BVHs"):
//   flat_cert <scratch_dir> <seed> <rays_per_scene> <generated_scenes> [scene.json ...]
// Every scene is loaded and compiled by the product (scene.cpp, compile.cpp). For a scene that got a flat
// program, both walks are executed for every ray as the kernel executes them for one lane (render.hip
// trace_linear: the same step semantics, operation order and roundings; -ffp-contract=off):
//   * the BVH program (lin_wide): slab test per node, skip on a miss;
//   * the flat program (flat_wide): no node test; the entry rule at every transform step, the end rule on
//     the winner's certificate box, uncertified when the world ray's reciprocal is not finite.
// Counted per scene: rays, hits, certified and uncertified hits, "decided" = rays whose two walks' winners
// differ in primitive, t or interval key (the rays a slab test decides), and "bad" = certified rays among
// them. Any bad ray is printed and the exit status is 1.
// Scenes: the files on the command line; generated scenes of 2 to 8 BVH leaves (walls with shared edges
// and corners, MakeBox boxes plain and rotated about y in different subtrees, thin boxes, integer
// coordinates, far-off coordinates where a quad's box padding is about 1 ulp of its plane); and the
// four-leaf scene in which the slab test decides every ray (a transformed box's model-space t culls the
// other subtree: Transform.cpp:13-20).
// Rays: through the scene's interior; aimed at edges and corners of the BVH nodes' boxes, on them and a
// few ulps beside; leaving a rounded hit point like a diffuse bounce (direction lengths 0.01 to 2); with
// zero, tiny and non-finite-reciprocal direction components; along box planes.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "scene.h"
#define RT2_BOXAA_FN inline
#include "boxaa.h"

using namespace rt2;

namespace {
uint32_t B(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}
float F(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
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
float Dot(V3 a, V3 b) {
  const float px = a.x * b.x, py = a.y * b.y, pz = a.z * b.z;
  return (px + py) + pz;
}
V3 Cross(V3 a, V3 b) { return V3{a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
bool Finite3(V3 v) { return std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z); }
float Gmax(float x, float y) { return (x < y) ? y : x; }
float Gmin(float x, float y) { return (y < x) ? y : x; }

// render.hip aabb_hit (AABB::Hit, AABB.hpp:34-47), for rays whose reciprocal is not finite
bool AabbHit(const float* lo, const float* hi, V3 o, V3 inv, float tmin, float tmax) {
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
uint32_t QuadAA(int k, const float* r, V3 o, V3 d, V3 inv, float& t_out) {
  const int a = (k + 1) % 3, b = (k + 2) % 3;
  const float dk = d[k];
  const float t = HostMath::div(r[0] - o[k], dk, inv[k]);
  const float pa = o[a] + d[a] * t, pb = o[b] + d[b] * t;
  t_out = t;
  return (B(pa - r[1]) | B(r[2] - pa) | B(pb - r[3])) | (B(r[4] - pb) | B(std::fabs(dk) - kAbove1e8));
}
// render.hip quad_cand_u on a QUAD record's 20 words, axis codes 0..3 (4..6 with the QUAD layout do not
// occur: the compiler gives such quads code K + 1)
bool QuadCand(uint32_t axis, const float* w, V3 o, V3 d, float& t_out) {
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

struct Result {
  uint32_t prim = kRefNone;
  float t = FLT_MAX;
  bool uncert = false;   // flat walk only
  bool xform = false;    // the winner lies under a transform (flat walk: from the certificate table)
};

// One lane's trace of a wide program (render.hip trace_linear), flat = the flat program with its certificate.
// mode = the launch's FlatMode. Returns false for a step the harness does not model.
bool Walk(const CompiledScene& c, bool flat, uint32_t mode, V3 wo, V3 wd, Result& out) {
  const std::vector<uint32_t>& prog = flat ? c.flat_wide : c.lin_wide;
  const float* recs = c.lind.data();
  V3 o = wo, d = wd;
  V3 inv{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
  const V3 winv = inv;
  bool fin = Finite3(inv);
  const bool wfin = fin;
  float tmax = FLT_MAX;
  uint32_t prim = kRefNone;
  bool xfail = false, xunc = false;
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
      if (flat) {
        const float lo[3] = {F(sw[4]), F(sw[5]), F(sw[6])}, hi[3] = {F(sw[7]), F(sw[8]), F(sw[9])};
        xfail = !FlatCertRule<HostMath>(lo, hi, o.x, o.y, o.z, inv.x, inv.y, inv.z, kTmin, tmax);
      }
      const float* m = recs + 4 * (size_t)off;
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
      fin = Finite3(inv);
      i++;
    } else if (kind == kXformExit) {
      if (sw[3] != kRefNone) return false;  // (flat programs and their BVH programs nest no transform)
      if (prim - make_ref(prim >> 28, off + (uint32_t)kXformRecords) < sw[1] - (off + (uint32_t)kXformRecords)) xunc = xfail;
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
  if (flat && prim != kRefNone) {
    const float* ct = &c.flat_cert[4 * (size_t)(prim & kOffsetMask)];
    out.xform = B(ct[3]) == kFlatCertXform;
    const bool end_ok = FlatCertRule<HostMath>(ct, ct + 4, wo.x, wo.y, wo.z, winv.x, winv.y, winv.z, kTmin, tmax);
    out.uncert = !wfin || mode == kFlatCertifyNothing || (out.xform ? xunc : !end_ok);
  }
  return true;
}

std::mt19937_64 rng;
float U(float lo, float hi) { return lo + (hi - lo) * (float)((rng() >> 11) * (1.0 / 9007199254740992.0)); }
float Ulps(float x, int n) {
  if (x == 0.0f) return n == 0 ? x : std::ldexp((float)n, -149);
  uint32_t b = B(x);
  if ((x > 0) == (n > 0)) b += (uint32_t)std::abs(n); else b -= (uint32_t)std::abs(n);
  return F(b);
}
V3 Dir(float len) {  // a direction of the given length
  V3 v;
  float l;
  do {
    v = V3{U(-1, 1), U(-1, 1), U(-1, 1)};
    l = Dot(v, v);
  } while (l > 1.0f || l < 1e-6f);
  const float s = len / std::sqrt(l);
  return V3{v.x * s, v.y * s, v.z * s};
}
float Len() { return std::exp(U(std::log(0.01f), std::log(2.0f))); }  // 0.01 .. 2, what the diffuse scatter produces

struct Tally {
  long rays = 0, hits = 0, cert = 0, uncert = 0, decided = 0, decided_uncert = 0, bad = 0, nonfinite = 0;
};

bool Compile(const std::string& path, CompiledScene& c) {
  Scene s;
  std::string err;
  if (!LoadScene(path, 1, s, err) || !CompileScene(s, c, err)) {
    fprintf(stderr, "%s: %s\n", path.c_str(), err.c_str());
    return false;
  }
  return true;
}

// The flat program's structure against the BVH program's (compile.cpp): the same leaf steps in the same
// order, the wide words bit copies of lind, every certificate box a bit copy of a BVH node's record whose
// range holds the leaf.
bool CheckProgram(const CompiledScene& c) {
  const size_t n = c.lin.size() / 4, m = c.flat_wide.size() / 16 - 1;
  if (c.flat_cert.size() != c.lind.size() || c.flat_wide[16 * m] != kProgramEnd) return false;
  std::vector<std::pair<size_t, size_t>> open;
  size_t j = 0;
  bool in_xf = false;
  for (size_t i = 0; i < n; i++) {
    while (!open.empty() && i >= open.back().second) open.pop_back();
    const uint32_t kind = c.lin[4 * i];
    if (kind == kBvh) {
      open.emplace_back(i, c.lin[4 * i + 1]);
      continue;
    }
    if (j >= m || open.empty()) return false;
    const uint32_t* w = &c.flat_wide[16 * j];
    if (w[0] != kind || w[2] != c.lin[4 * i + 2]) return false;
    const float* box = &c.lind[4 * (size_t)c.lin[4 * open.back().first + 2]];
    if (kind == kXform) {
      if (memcmp(&w[4], box, 12) || memcmp(&w[7], box + 4, 12)) return false;
      in_xf = true;
    } else if (kind == kQuad) {
      const float* ct = &c.flat_cert[4 * (size_t)w[2]];
      if (in_xf ? B(ct[3]) != kFlatCertXform : (memcmp(ct, box, 12) || memcmp(ct + 4, box + 4, 12) || B(ct[3]) != 0u))
        return false;
      if (memcmp(&w[4], &c.lind[4 * (size_t)w[2]], 48)) return false;
    } else if (kind == kXformExit) {
      in_xf = false;
    } else {
      return false;
    }
    j++;
  }
  if (j != m) return false;
  // runs: a quad step's run covers consecutive quad steps with contiguous records
  for (j = 0; j < m; j++) {
    const uint32_t* w = &c.flat_wide[16 * j];
    if (w[0] != kQuad) continue;
    const uint32_t run = w[3] & kRunLenMask;
    for (uint32_t k = 1; k < run; k++)
      if (j + k >= m || c.flat_wide[16 * (j + k)] != kQuad || c.flat_wide[16 * (j + k) + 2] != w[2] + k * (uint32_t)kQuadRecords)
        return false;
  }
  return true;
}

struct Box6 {
  float lo[3], hi[3];
};
std::vector<Box6> NodeBoxes(const CompiledScene& c) {
  std::vector<Box6> out;
  for (size_t i = 0; i < c.lin.size() / 4; i++) {
    if (c.lin[4 * i] != kBvh) continue;
    const float* r = &c.lind[4 * (size_t)c.lin[4 * i + 2]];
    out.push_back(Box6{{r[0], r[1], r[2]}, {r[4], r[5], r[6]}});
  }
  return out;
}

void Report(const char* what, const V3& o, const V3& d, const Result& a, const Result& b) {
  fprintf(stderr, "%s\n o = (%a %a %a) d = (%a %a %a)\n bvh: prim %08x t %a\n flat: prim %08x t %a uncert %d xform %d\n", what,
          o.x, o.y, o.z, d.x, d.y, d.z, a.prim, a.t, b.prim, b.t, (int)b.uncert, (int)b.xform);
}

// Both walks of one ray; returns false on a certified disagreement or an unmodelled step.
bool OneRay(const CompiledScene& c, V3 o, V3 d, Tally& t, Result* bvh_out = nullptr) {
  if (!Finite3(o) || !Finite3(d)) return true;
  Result a, b;
  if (!Walk(c, false, kFlatOn, o, d, a) || !Walk(c, true, c.flat_mode, o, d, b)) {
    fprintf(stderr, "a step the harness does not model\n");
    return false;
  }
  if (bvh_out) *bvh_out = a;
  t.rays++;
  const V3 inv{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
  if (!Finite3(inv)) t.nonfinite++;
  if (b.prim != kRefNone) {
    t.hits++;
    (b.uncert ? t.uncert : t.cert)++;
  }
  const bool differ = a.prim != b.prim || B(a.t) != B(b.t);  // (the interval key is bits(t) - bits(tmin))
  if (differ) {
    t.decided++;
    if (b.uncert) {
      t.decided_uncert++;
    } else {
      t.bad++;
      Report("CERTIFIED RAY DISAGREES", o, d, a, b);
      return false;
    }
  }
  return true;
}

bool RunRays(const CompiledScene& c, long nray, Tally& t) {
  const std::vector<Box6> boxes = NodeBoxes(c);
  if (boxes.empty()) return false;
  const Box6& root = boxes[0];
  float size = 0;
  for (int k = 0; k < 3; k++) size = std::max(size, root.hi[k] - root.lo[k]);
  for (long r = 0; r < nray; r++) {
    const int cls = (int)(r % 6);
    V3 o, d;
    auto inside = [&] { return V3{U(root.lo[0], root.hi[0]), U(root.lo[1], root.hi[1]), U(root.lo[2], root.hi[2])}; };
    const Box6& bx = boxes[rng() % boxes.size()];
    if (cls == 0) {  // through the interior
      o = inside();
      d = Dir(Len());
    } else if (cls == 1 || cls == 2) {  // aimed at an edge / corner of a node's box, on it or a few ulps beside
      float p[3];
      for (int k = 0; k < 3; k++) p[k] = U(bx.lo[k], bx.hi[k]);
      const int k1 = (int)(rng() % 3), k2 = (k1 + 1 + (int)(rng() % 2)) % 3;
      p[k1] = Ulps((rng() % 2) ? bx.hi[k1] : bx.lo[k1], (int)(rng() % 7) - 3);
      p[k2] = Ulps((rng() % 2) ? bx.hi[k2] : bx.lo[k2], (int)(rng() % 7) - 3);
      if (cls == 2) {
        const int k3 = 3 - k1 - k2;
        p[k3] = Ulps((rng() % 2) ? bx.hi[k3] : bx.lo[k3], (int)(rng() % 7) - 3);
      }
      const V3 v = Dir(1.0f);
      const float L = size * std::ldexp(U(0.5f, 1.0f), (int)(rng() % 12) - 8);
      o = (rng() % 2) ? inside() : V3{p[0] + L * v.x, p[1] + L * v.y, p[2] + L * v.z};
      d = V3{p[0] - o.x, p[1] - o.y, p[2] - o.z};
      const float l = std::sqrt(Dot(d, d));
      if (!(l > 0)) continue;
      const float s = Len() / l;
      d = V3{d.x * s, d.y * s, d.z * s};
    } else if (cls == 3) {  // a diffuse bounce: leaving the rounded hit point of a ray through the interior
      Result h;
      o = inside();
      d = Dir(Len());
      if (!OneRay(c, o, d, t, &h)) return false;
      if (h.prim == kRefNone) continue;
      // (a hit under a transform carries a model-space t, in units of the normalized direction)
      const float tw = B(c.flat_cert[4 * (size_t)(h.prim & kOffsetMask) + 3]) == kFlatCertXform ? h.t / std::sqrt(Dot(d, d)) : h.t;
      o = V3{o.x + d.x * tw, o.y + d.y * tw, o.z + d.z * tw};
      d = Dir(Len());
    } else if (cls == 4) {  // zero, tiny and non-finite-reciprocal components
      o = inside();
      d = Dir(Len());
      const int k = (int)(rng() % 3);
      const int kindz = (int)(rng() % 4);
      float z = kindz == 0 ? 0.0f : kindz == 1 ? -0.0f : kindz == 2 ? std::ldexp(1.0f, -(int)(rng() % 40) - 100) : 1e-39f;
      if (rng() % 2) z = -z;
      (k == 0 ? d.x : k == 1 ? d.y : d.z) = z;
      if (rng() % 4 == 0) (k == 0 ? d.y : d.x) = 0.0f;
    } else {  // along a plane of a node's box: the origin on the plane, no motion across it
      o = inside();
      d = Dir(Len());
      const int k = (int)(rng() % 3);
      const float pl = Ulps((rng() % 2) ? bx.hi[k] : bx.lo[k], (int)(rng() % 5) - 2);
      (k == 0 ? o.x : k == 1 ? o.y : o.z) = pl;
      if (rng() % 2) (k == 0 ? d.x : k == 1 ? d.y : d.z) = (rng() % 2) ? 0.0f : std::ldexp(U(-1, 1), -30);
    }
    if (!OneRay(c, o, d, t)) return false;
  }
  return true;
}

void Print(const std::string& name, const CompiledScene& c, const Tally& t) {
  printf("%s flat=%d steps=%d rays=%ld hits=%ld certified=%ld uncertified=%ld nonfinite=%ld decided=%ld decided_uncertified=%ld bad=%ld\n",
         name.c_str(), c.flat_wide.empty() ? 0 : 1, c.flat_steps, t.rays, t.hits, t.cert, t.uncert, t.nonfinite, t.decided,
         t.decided_uncert, t.bad);
}

bool WriteFile(const std::string& path, const std::string& text) {
  FILE* f = fopen(path.c_str(), "w");
  if (!f) return false;
  fputs(text.c_str(), f);
  fclose(f);
  return true;
}
std::string Vec(float x, float y, float z) {
  char b[128];
  snprintf(b, sizeof b, "[%.9g, %.9g, %.9g]", x, y, z);
  return b;
}
const char* kHead = "{\"camera\": {\"center\": [0, 0, -10], \"look_at\": [0, 0, 0]}, \"materials\": [{\"type\": "
                    "\"lambertian\", \"albedo\": [0.5, 0.5, 0.5]}], \"primitives\": [";

// The issue's four-leaf scene: a unit-scale box rotated +10 degrees about y at the origin, two 30 x 30 quads
// at x = 200 and x = 400, the same box rotated -10 degrees at (600, 0, 0).
std::string FourLeafScene() {
  std::string js = kHead;
  js += "{\"type\": \"box\", \"a\": [0, 0, 0], \"b\": [165, 165, 165], \"material\": 0}, ";
  js += "{\"type\": \"quad\", \"q\": [200, 60, 60], \"u\": [0, 30, 0], \"v\": [0, 0, 30], \"material\": 0}, ";
  js += "{\"type\": \"quad\", \"q\": [400, 60, 60], \"u\": [0, 30, 0], \"v\": [0, 0, 30], \"material\": 0}, ";
  js += "{\"type\": \"box\", \"a\": [0, 0, 0], \"b\": [165, 165, 165], \"material\": 0}], \"scene\": [";
  js += "{\"primitive\": 0, \"transform\": {\"translation\": [0, 0, 0], \"rotation\": [10, 0, 1, 0]}}, ";
  js += "{\"primitive\": 1}, {\"primitive\": 2}, ";
  js += "{\"primitive\": 3, \"transform\": {\"translation\": [600, 0, 0], \"rotation\": [-10, 0, 1, 0]}}]}";
  return js;
}

// A generated scene of `leaves` BVH leaves around `origin` at scale `sc`: walls on a shared grid of plane
// coordinates (shared edges and corners), plain boxes, thin boxes, boxes rotated about y.
std::string GeneratedScene(int leaves, float sc, const float origin[3], bool integer) {
  std::string prims, nodes;
  const float grid[4] = {0.0f, 1.0f, 2.0f, 3.0f};
  for (int i = 0; i < leaves; i++) {
    const int kind = (int)(rng() % 5);
    auto co = [&](int k, float g) {
      float v = origin[k] + sc * g;
      return integer ? std::round(v) : v;
    };
    char buf[512];
    if (kind <= 1) {  // a wall: one plane coordinate and a rectangle of the grid
      const int k = (int)(rng() % 3), a = (k + 1) % 3, b = (k + 2) % 3;
      float q[3], u[3] = {0, 0, 0}, v[3] = {0, 0, 0};
      const int ga = (int)(rng() % 3), gb = (int)(rng() % 3);
      q[k] = co(k, grid[rng() % 4]);
      q[a] = co(a, grid[ga]);
      q[b] = co(b, grid[gb]);
      u[a] = co(a, grid[ga + 1 + (int)(rng() % (3 - ga))]) - q[a];
      v[b] = co(b, grid[gb + 1 + (int)(rng() % (3 - gb))]) - q[b];
      snprintf(buf, sizeof buf, "{\"type\": \"quad\", \"q\": %s, \"u\": %s, \"v\": %s, \"material\": 0}", Vec(q[0], q[1], q[2]).c_str(),
               Vec(u[0], u[1], u[2]).c_str(), Vec(v[0], v[1], v[2]).c_str());
      nodes += std::string(i ? ", " : "") + "{\"primitive\": " + std::to_string(i) + "}";
    } else {
      float a[3], e[3];
      for (int k = 0; k < 3; k++) {
        a[k] = kind == 4 ? 0.0f : co(k, U(0.0f, 2.0f));
        e[k] = sc * U(0.2f, 1.0f);
        if (integer) e[k] = std::round(e[k]) + 1.0f;
      }
      if (kind == 3) e[(int)(rng() % 3)] *= 1e-4f;  // thin
      snprintf(buf, sizeof buf, "{\"type\": \"box\", \"a\": %s, \"b\": %s, \"material\": 0}", Vec(a[0], a[1], a[2]).c_str(),
               Vec(a[0] + e[0], a[1] + e[1], a[2] + e[2]).c_str());
      if (kind == 4) {  // unit scale, rotated about y, placed on the grid
        char tb[256];
        snprintf(tb, sizeof tb, "{\"primitive\": %d, \"transform\": {\"translation\": %s, \"rotation\": [%.9g, 0, 1, 0]}}", i,
                 Vec(co(0, U(0.0f, 2.5f)), co(1, U(0.0f, 2.5f)), co(2, U(0.0f, 2.5f))).c_str(), U(-40.0f, 40.0f));
        nodes += std::string(i ? ", " : "") + tb;
      } else {
        nodes += std::string(i ? ", " : "") + "{\"primitive\": " + std::to_string(i) + "}";
      }
    }
    prims += std::string(i ? ", " : "") + buf;
  }
  return std::string(kHead) + prims + "], \"scene\": [" + nodes + "]}";
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: flat_cert <scratch_dir> <seed> <rays_per_scene> <generated_scenes> [scene.json ...]\n");
    return 2;
  }
  const std::string dir = argv[1];
  rng.seed(strtoull(argv[2], nullptr, 10));
  const long nray = atol(argv[3]);
  const int ngen = atoi(argv[4]);
  unsetenv("RT2_FLAT_BVH");
  int rc = 0;
  // the committed scenes on the command line
  for (int i = 5; i < argc; i++) {
    CompiledScene c;
    if (!Compile(argv[i], c)) return 2;
    Tally t;
    if (!c.flat_wide.empty()) {
      if (!CheckProgram(c)) {
        fprintf(stderr, "%s: the flat program is not the BVH program's leaf steps\n", argv[i]);
        return 1;
      }
      if (!RunRays(c, nray, t)) rc = 1;
    }
    std::string name = argv[i];
    name = name.substr(name.find_last_of('/') + 1);
    Print("scene:" + name, c, t);
    if (rc) return rc;
  }
  // generated scenes
  Tally gen;
  int gen_flat = 0;
  for (int g = 0; g < ngen; g++) {
    const int leaves = 2 + g % 7;
    const int cls = (g / 7) % 4;
    const float sc = cls == 0 ? 1.0f : cls == 1 ? 185.0f : cls == 2 ? 555.0f : 1.0f;
    const float far = cls == 3 ? 16384.0f : (cls == 2 ? 0.0f : U(-4.0f, 4.0f) * sc);
    const float origin[3] = {far, cls == 3 ? 4096.0f : 0.0f, -far};
    const std::string path = dir + "/flat_cert_gen.json";
    if (!WriteFile(path, GeneratedScene(leaves, sc, origin, cls == 2))) return 2;
    CompiledScene c;
    if (!Compile(path, c)) return 2;
    if (c.flat_wide.empty()) continue;
    gen_flat++;
    if (!CheckProgram(c)) {
      fprintf(stderr, "generated scene %d: the flat program is not the BVH program's leaf steps\n", g);
      return 1;
    }
    if (!RunRays(c, nray, gen)) {
      fprintf(stderr, "generated scene %d (%d leaves) kept at %s\n", g, leaves, path.c_str());
      return 1;
    }
  }
  {
    CompiledScene none;
    none.flat_steps = gen_flat;
    none.flat_wide.assign(gen_flat ? 16 : 0, 0u);
    Print("generated", none, gen);
  }
  // the four-leaf scene with its rays: x = 1000, direction (-s, ~0, ~0), s in {0.1, 0.01}
  {
    const std::string path = dir + "/flat_cert_four.json";
    if (!WriteFile(path, FourLeafScene())) return 2;
    CompiledScene c;
    if (!Compile(path, c)) return 2;
    Tally t;
    if (c.flat_wide.empty() || !CheckProgram(c)) {
      fprintf(stderr, "the four-leaf scene got no flat program\n");
      return 1;
    }
    for (int k = 0; k < 160000; k++) {
      const float s = (k & 1) ? 0.1f : 0.01f;
      const V3 o{1000.0f, U(5.0f, 160.0f), U(40.0f, 120.0f)};
      const V3 d{-s, U(-1e-4f, 1e-4f) * s, U(-1e-4f, 1e-4f) * s};
      if (!OneRay(c, o, d, t)) return 1;
    }
    Print("four_leaf", c, t);
  }
  return rc;
}
