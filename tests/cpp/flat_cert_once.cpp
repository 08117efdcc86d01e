// Host check that the flat walk's certificate, evaluated once per trace, decides what the entry rule and the
// end rule decided (rt2_layout.h "Flat program", boxaa.h FlatCertRule, DESIGN.md §4 "Flat walk of small BVHs"):
//   flat_cert_once <scratch_dir> <seed> <rays_per_scene> <generated_scenes> [scene.json ...]
// Every scene is loaded and compiled by the product (scene.cpp, compile.cpp). For a scene that got a flat
// program:
//   * table check: every quad step between a kXform step and its exit has, in the certificate table, that
//     transform's certificate box (words 4-9 of the transform's wide entry) bit for bit, beside its
//     kFlatCertXform flag; every other quad's row has no flag;
//   * per-ray check: the flat program is walked twice for every ray, as the kernel walks it for one lane
//     (render.hip trace_linear: the same step semantics, operation order and roundings; -ffp-contract=off).
//     kEager restates the earlier evaluation: FlatCertRule at every kXform step on the step's own box with
//     the lane's tmax there (xfail), carried to the exit when the closest hit lies under the transform (xunc),
//     and the end rule on the winner's row with T = its t, of which one verdict is read by the row's flag.
//     kLazy is the kernel's: t_entry kept at the kXform step, t_keep = t_entry at such an exit, and one rule
//     after the walk on the winner's row with T = flag ? t_keep : t. Both must return the same primitive,
//     the same t and the same `uncertified` for every ray.
// Printed per scene: rays, hits, rule_uncert_xform / rule_uncert_world = hits with a finite world reciprocal
// that the rule leaves uncertified, under a transform / in world space, nonfinite, table_rows, bad. Any bad
// ray is printed and the exit status is 1.
// Scenes and rays are drawn as tests/cpp/flat_cert.cpp draws them: the files on the command line; generated
// scenes of 2 to 8 BVH leaves; the four-leaf scene with its rays.
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

// render.hip quad_aa<K>: the rejection word of a QUADAA record
uint32_t QuadAA(int k, const float* r, V3 o, V3 d, V3 inv, float& t_out) {
  const int a = (k + 1) % 3, b = (k + 2) % 3;
  const float dk = d[k];
  const float t = HostMath::div(r[0] - o[k], dk, inv[k]);
  const float pa = o[a] + d[a] * t, pb = o[b] + d[b] * t;
  t_out = t;
  return (B(pa - r[1]) | B(r[2] - pa) | B(pb - r[3])) | (B(r[4] - pb) | B(std::fabs(dk) - kAbove1e8));
}
// render.hip quad_cand_u on a QUAD record's 20 words, axis codes 0..3
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
  bool uncert = false;
  bool xform = false;  // the winner's row carries kFlatCertXform
  bool wfin = false;   // the world ray's reciprocal is finite
};

enum Cert { kEager, kLazy };

// One lane's trace of the flat program (render.hip trace_linear with kFlat), with the certificate evaluated
// eagerly (entry rule at entry, end rule at the end) or lazily (one rule after the walk). Returns false for a
// step the harness does not model.
template <Cert kCert>
bool Walk(const CompiledScene& c, uint32_t mode, V3 wo, V3 wd, Result& out) {
  const std::vector<uint32_t>& prog = c.flat_wide;
  const float* recs = c.lind.data();
  V3 o = wo, d = wd;
  V3 inv{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
  const V3 winv = inv;
  const bool wfin = Finite3(inv);
  float tmax = FLT_MAX;
  uint32_t prim = kRefNone;
  bool xfail = false, xunc = false;            // kEager
  float t_entry = FLT_MAX, t_keep = FLT_MAX;   // kLazy
  uint32_t i = 0;
  for (size_t guard = 0; guard < 100000; guard++) {
    const uint32_t* sw = &prog[16 * (size_t)i];
    const uint32_t kind = sw[0], off = sw[2];
    if (kind == kProgramEnd) break;
    if (kind == kQuad) {
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
      if (kCert == kEager) {
        // the entry rule on the step's own box with the ray the lane carries here (the world ray: flat
        // programs nest no transform) and T = the lane's tmax here
        const float lo[3] = {F(sw[4]), F(sw[5]), F(sw[6])}, hi[3] = {F(sw[7]), F(sw[8]), F(sw[9])};
        xfail = !FlatCertRule<HostMath>(lo, hi, o.x, o.y, o.z, inv.x, inv.y, inv.z, kTmin, tmax);
      } else {
        t_entry = tmax;
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
      i++;
    } else if (kind == kXformExit) {
      if (sw[3] != kRefNone) return false;  // (flat programs nest no transform)
      if (prim - make_ref(prim >> 28, off + (uint32_t)kXformRecords) < sw[1] - (off + (uint32_t)kXformRecords)) {
        if (kCert == kEager) xunc = xfail; else t_keep = t_entry;
      }
      o = wo;
      d = wd;
      inv = winv;
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
  if (prim != kRefNone) {
    const float* ct = &c.flat_cert[4 * (size_t)(prim & kOffsetMask)];
    out.xform = B(ct[3]) == kFlatCertXform;
    if (kCert == kEager) {
      const bool end_ok = FlatCertRule<HostMath>(ct, ct + 4, wo.x, wo.y, wo.z, winv.x, winv.y, winv.z, kTmin, tmax);
      out.uncert = !wfin || mode == kFlatCertifyNothing || (out.xform ? xunc : !end_ok);
    } else {
      const float T = out.xform ? t_keep : tmax;
      const bool rule = FlatCertRule<HostMath>(ct, ct + 4, wo.x, wo.y, wo.z, winv.x, winv.y, winv.z, kTmin, T);
      out.uncert = !wfin || mode == kFlatCertifyNothing || !rule;
    }
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
  long rays = 0, hits = 0, rule_uncert_xform = 0, rule_uncert_world = 0, nonfinite = 0, table_rows = 0, bad = 0;
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

// The certificate table against the flat program: a quad step between a kXform step and its exit holds that
// step's words 4-9 (lo.xyz | flag) (hi.xyz | 0); a quad step outside any transform holds no flag.
bool CheckTable(const CompiledScene& c, Tally& t) {
  const size_t m = c.flat_wide.size() / 16 - 1;
  if (c.flat_cert.size() != c.lind.size() || c.flat_wide[16 * m] != kProgramEnd) return false;
  const uint32_t* xf = nullptr;
  for (size_t j = 0; j < m; j++) {
    const uint32_t* w = &c.flat_wide[16 * j];
    if (w[0] == kXform) {
      if (xf) return false;
      xf = w;
    } else if (w[0] == kXformExit) {
      if (!xf) return false;
      xf = nullptr;
    } else if (w[0] == kQuad) {
      const float* ct = &c.flat_cert[4 * (size_t)w[2]];
      if (xf) {
        if (memcmp(ct, &xf[4], 12) || memcmp(ct + 4, &xf[7], 12) || B(ct[3]) != kFlatCertXform || B(ct[7]) != 0u) {
          fprintf(stderr, "step %zu: the row of a quad under a transform is not the transform's certificate box\n", j);
          return false;
        }
        t.table_rows++;
      } else if (B(ct[3]) != 0u) {
        return false;
      }
    } else {
      return false;
    }
  }
  return xf == nullptr;
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

// Both evaluations on one ray; returns false on a disagreement or an unmodelled step.
bool OneRay(const CompiledScene& c, V3 o, V3 d, Tally& t, Result* out = nullptr) {
  if (!Finite3(o) || !Finite3(d)) return true;
  Result a, b;
  if (!Walk<kEager>(c, c.flat_mode, o, d, a) || !Walk<kLazy>(c, c.flat_mode, o, d, b)) {
    fprintf(stderr, "a step the harness does not model\n");
    return false;
  }
  if (out) *out = b;
  t.rays++;
  if (!b.wfin) t.nonfinite++;
  if (b.prim != kRefNone) {
    t.hits++;
    if (b.uncert && b.wfin) (b.xform ? t.rule_uncert_xform : t.rule_uncert_world)++;
  }
  if (a.prim != b.prim || B(a.t) != B(b.t) || a.uncert != b.uncert || a.xform != b.xform) {
    t.bad++;
    fprintf(stderr, "THE TWO EVALUATIONS DISAGREE\n o = (%a %a %a) d = (%a %a %a)\n eager: prim %08x t %a uncert %d\n"
            " lazy: prim %08x t %a uncert %d xform %d\n", o.x, o.y, o.z, d.x, d.y, d.z, a.prim, a.t, (int)a.uncert, b.prim,
            b.t, (int)b.uncert, (int)b.xform);
    return false;
  }
  return true;
}

// The ray classes of flat_cert.cpp RunRays.
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
      const float tw = h.xform ? h.t / std::sqrt(Dot(d, d)) : h.t;
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

void Print(const std::string& name, int flat, int steps, const Tally& t) {
  printf("%s flat=%d steps=%d rays=%ld hits=%ld rule_uncert_xform=%ld rule_uncert_world=%ld nonfinite=%ld table_rows=%ld bad=%ld\n",
         name.c_str(), flat, steps, t.rays, t.hits, t.rule_uncert_xform, t.rule_uncert_world, t.nonfinite, t.table_rows, t.bad);
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

// flat_cert.cpp's four-leaf scene: a unit-scale box rotated +10 degrees about y at the origin, two 30 x 30
// quads at x = 200 and x = 400, the same box rotated -10 degrees at (600, 0, 0).
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

// flat_cert.cpp's generated scene of `leaves` BVH leaves around `origin` at scale `sc`: walls on a shared grid
// of plane coordinates, plain boxes, thin boxes, boxes rotated about y.
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
    fprintf(stderr, "usage: flat_cert_once <scratch_dir> <seed> <rays_per_scene> <generated_scenes> [scene.json ...]\n");
    return 2;
  }
  const std::string dir = argv[1];
  rng.seed(strtoull(argv[2], nullptr, 10));
  const long nray = atol(argv[3]);
  const int ngen = atoi(argv[4]);
  unsetenv("RT2_FLAT_BVH");
  // the committed scenes on the command line
  for (int i = 5; i < argc; i++) {
    CompiledScene c;
    if (!Compile(argv[i], c)) return 2;
    std::string name = argv[i];
    name = name.substr(name.find_last_of('/') + 1);
    Tally t;
    if (c.flat_wide.empty()) {
      fprintf(stderr, "%s got no flat program\n", argv[i]);
      return 1;
    }
    if (!CheckTable(c, t)) {
      fprintf(stderr, "%s: the certificate table does not hold the transforms' boxes\n", argv[i]);
      return 1;
    }
    const bool ok = RunRays(c, nray, t);
    Print("scene:" + name, 1, c.flat_steps, t);
    if (!ok) return 1;
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
    const std::string path = dir + "/flat_cert_once_gen.json";
    if (!WriteFile(path, GeneratedScene(leaves, sc, origin, cls == 2))) return 2;
    CompiledScene c;
    if (!Compile(path, c)) return 2;
    if (c.flat_wide.empty()) continue;
    gen_flat++;
    if (!CheckTable(c, gen)) {
      fprintf(stderr, "generated scene %d: the certificate table does not hold the transforms' boxes\n", g);
      return 1;
    }
    if (!RunRays(c, nray, gen)) {
      fprintf(stderr, "generated scene %d (%d leaves) kept at %s\n", g, leaves, path.c_str());
      return 1;
    }
  }
  Print("generated", gen_flat ? 1 : 0, gen_flat, gen);
  // the four-leaf scene with its rays: x = 1000, direction (-s, ~0, ~0), s in {0.1, 0.01}
  {
    const std::string path = dir + "/flat_cert_once_four.json";
    if (!WriteFile(path, FourLeafScene())) return 2;
    CompiledScene c;
    if (!Compile(path, c)) return 2;
    Tally t;
    if (c.flat_wide.empty() || !CheckTable(c, t)) {
      fprintf(stderr, "the four-leaf scene got no flat program with the transforms' boxes in its table\n");
      return 1;
    }
    for (int k = 0; k < 160000; k++) {
      const float s = (k & 1) ? 0.1f : 0.01f;
      const V3 o{1000.0f, U(5.0f, 160.0f), U(40.0f, 120.0f)};
      const V3 d{-s, U(-1e-4f, 1e-4f) * s, U(-1e-4f, 1e-4f) * s};
      if (!OneRay(c, o, d, t)) return 1;
    }
    Print("four_leaf", 1, c.flat_steps, t);
  }
  return 0;
}
