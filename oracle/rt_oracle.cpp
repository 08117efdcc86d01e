// rt_oracle.cpp — CPU restatement of the reference render loop (tonadr1022/Raytrace2
// src/cpu_raytrace + src/Serialize.cpp). TEST INFRASTRUCTURE ONLY.
//
// Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this library,
// and only as the checker / the timed CPU baseline — never as the product path.
//
// Parity status: PINNED TO THE COMPILED REFERENCE for everything in src/cpu_raytrace. oracle/Makefile's
// ref target compiles the reference's own src/cpu_raytrace/*.cpp (RayTracer.cpp included) against the
// stand-ins of oracle/refshim into oracle/_ref/librt2_ref.so, and tests/test_reference_build.py compares
// this restatement with it bit for bit under CTL_REF_MATH, the reference fed this file's uniforms: the
// streams, the camera, closest hits on thousands of rays per scene, whole paths through
// RayTracer::Update and the Perlin textures, with zero differing words on the nine parity scenes.
// Besides: (a) the Philox4x32-10 known-answer vectors, (b) hand-derived known answers for the
// deterministic functions (tests/test_oracle_kat.py) and (c) a statistical comparison of converged
// renders against the reference's screenshots (tests/test_reference_pin.py).
// Still restated, not pinned: glm's arithmetic (lines "glm-like value types" below and the stand-in
// oracle/refshim/glm/rt2_glm.hpp are two writings of glm's published operation order; glm itself is not
// available) and Serialize.cpp (LoadScene below and ref_driver.cpp's loader are two independent
// restatements that agree). See DESIGN.md §2.
//
// Deliberate, documented deviations from the reference (all RNG-related, Finding 2 of SURVEY.md):
//  * RandReal(): Philox4x32-10 counter stream keyed by (seed, pixel, frame) instead of the
//    thread_local std::minstd_rand seeded from std::random_device (Math.hpp:9-13).
//  * Perlin tables are drawn from a Philox stream keyed by (seed, noise texture ordinal).
//  * log() in ConstantMedium is the shared float polynomial LogU (within 1 ulp; the reference calls
//    glibc logf, itself within an ulp); sin() in the marble texture is the shared float
//    restatement SinF (within 9e-8 of sin for |x| <= 5000; the reference calls sinf).
//  * pow(1-cos, 5) in Schlick is an explicit double multiplication chain (reference: std::pow).
//  * RandUnitVec3 / RandInUnitDisk draw their (identical) distributions by inverse-CDF maps
//    instead of rejection loops, with a shared polynomial sin/cos (see CosSin2Pi).
//  * Missing "rotation" in a transform is the identity quaternion (reference: uninitialised
//    glm::quat, undefined behaviour; Serialize.cpp:114).
// Compile with -ffp-contract=off: every float op below is rounded individually, like the
// reference's x86-64 (non-FMA) build.

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <thread>
#include <utility>
#include <vector>


namespace oracle {

using real = float;
// Controls (tests only, oracle_set_controls): each bit REMOVES one of the reference's quirks, to
// measure whether the statistical pins against the reference's screenshots can tell the faithful
// restatement from one without that quirk (DESIGN.md §2 "Power of the pin"). 0 = faithful.
//   1: transformed children report world-space t (model-space direction left unnormalised) instead
//      of the model-space t of Transform.cpp:13-20,75-88
//   2: a span-1 BVH leaf is tested once, not twice (BVH.cpp:18-20, 50-55)
//   4: kInfinity = +inf instead of FLT_MAX (Defs.hpp:17)
// and one bit that RESTORES the reference's own sampling and libm calls where the restatement
// deviates on purpose (DESIGN.md §2 "Deliberate deviations"), to measure those deviations:
//   8: RandInUnitSphere / RandInUnitDisk by rejection on the same Philox stream (Math.hpp:26-43),
//      std::log(float) in ConstantMedium (ConstantMedium.cpp:42), std::sin(float) in the marble
//      texture (Texture.cpp:16), glm::pow(1 - cos, 5) = std::pow(double, int) in Schlick
//      (Material.cpp:24; glm's scalar pow is std::pow, and (float, int) promotes to double)
// and one bit that removes no quirk but a pruning step, to measure what the images can see of it:
//   16: BVHNode::Hit skips its slab test (BVH.cpp:51) and visits both children: all leaves in pre-order
//       with a running tmax, the product's flat walk without its certificate (DESIGN.md §4 "Flat walk of
//       small BVHs"). The slab test is no pure optimisation: a transformed child reports model-space t, so
//       a hit's tmax can cull the subtree that holds a nearer surface. The bvh counter still counts.
enum : int { kCtlWorldT = 1, kCtlSingleLeaf = 2, kCtlInf = 4, kCtlRefMath = 8, kCtlNoSlab = 16 };
static int g_controls = 0;
#define kInfinity ((g_controls & kCtlInf) ? (real)INFINITY : (real)FLT_MAX)  // Defs.hpp:17

// ----------------------------------------------------------------------------------------------
// glm-like value types (Appendix C of SURVEY.md). Column-major mat4 like glm.
struct vec2 {
  float x{0}, y{0};
};
struct vec3 {
  float x{0}, y{0}, z{0};
  vec3() = default;
  vec3(float a, float b, float c) : x(a), y(b), z(c) {}
  explicit vec3(float s) : x(s), y(s), z(s) {}
  float& operator[](int i) { return i == 0 ? x : (i == 1 ? y : z); }
  float operator[](int i) const { return i == 0 ? x : (i == 1 ? y : z); }
};
struct vec4 {
  float x{0}, y{0}, z{0}, w{0};
  float& operator[](int i) { return i == 0 ? x : (i == 1 ? y : (i == 2 ? z : w)); }
  float operator[](int i) const { return i == 0 ? x : (i == 1 ? y : (i == 2 ? z : w)); }
};
inline vec3 operator+(vec3 a, vec3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline vec3 operator-(vec3 a, vec3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline vec3 operator*(vec3 a, vec3 b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
inline vec3 operator*(vec3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
inline vec3 operator*(float s, vec3 a) { return {s * a.x, s * a.y, s * a.z}; }
inline vec3 operator/(vec3 a, float s) { return {a.x / s, a.y / s, a.z / s}; }
inline vec3 operator-(vec3 a) { return {-a.x, -a.y, -a.z}; }
inline vec4 operator*(vec4 a, vec4 b) { return {a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w}; }
inline vec4 operator*(vec4 a, float s) { return {a.x * s, a.y * s, a.z * s, a.w * s}; }
inline vec4 operator+(vec4 a, vec4 b) { return {a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }
inline vec4 operator-(vec4 a, vec4 b) { return {a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w}; }
// glm compute_dot<vec3>: tmp = a*b; return (tmp.x + tmp.y) + tmp.z
inline float dot(vec3 a, vec3 b) {
  vec3 t = a * b;
  return (t.x + t.y) + t.z;
}
inline vec3 cross(vec3 x, vec3 y) {
  return {x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y};
}
// glm::normalize = v * inversesqrt(dot(v, v)), inversesqrt(x) = 1 / sqrt(x)
inline vec3 normalize(vec3 v) { return v * (1.0f / std::sqrt(dot(v, v))); }
inline float length(vec3 v) { return std::sqrt(dot(v, v)); }
// glm scalar min/max: max(x,y) = (x < y) ? y : x ; min(x,y) = (y < x) ? y : x
inline float gmax(float x, float y) { return (x < y) ? y : x; }
inline float gmin(float x, float y) { return (y < x) ? y : x; }
inline float radians(float deg) { return deg * 0.01745329251994329576923690768489f; }

struct mat4 {
  vec4 c[4];
  static mat4 identity() {
    mat4 m;
    m.c[0] = {1, 0, 0, 0};
    m.c[1] = {0, 1, 0, 0};
    m.c[2] = {0, 0, 1, 0};
    m.c[3] = {0, 0, 0, 1};
    return m;
  }
  vec4& operator[](int i) { return c[i]; }
  const vec4& operator[](int i) const { return c[i]; }
};
// glm mat4 * vec4: (m0*v.x + m1*v.y) + (m2*v.z + m3*v.w)
inline vec4 mul(const mat4& m, vec4 v) {
  vec4 a0 = m[0] * v.x, a1 = m[1] * v.y, a2 = m[2] * v.z, a3 = m[3] * v.w;
  return (a0 + a1) + (a2 + a3);
}
inline vec3 xyz(vec4 v) { return {v.x, v.y, v.z}; }
// glm mat4 * mat4: Result[i] = ((A0*B[i][0] + A1*B[i][1]) + A2*B[i][2]) + A3*B[i][3]
inline mat4 mul(const mat4& a, const mat4& b) {
  mat4 r;
  for (int i = 0; i < 4; i++) {
    r[i] = ((a[0] * b[i][0] + a[1] * b[i][1]) + a[2] * b[i][2]) + a[3] * b[i][3];
  }
  return r;
}
// glm mat3(mat4) * vec3: row sums left to right
inline vec3 mul3(const mat4& m, vec3 v) {
  return {m[0][0] * v.x + m[1][0] * v.y + m[2][0] * v.z,
          m[0][1] * v.x + m[1][1] * v.y + m[2][1] * v.z,
          m[0][2] * v.x + m[1][2] * v.y + m[2][2] * v.z};
}
// mat3(transpose(M)) * v  ==  rows of M's upper 3x3 dotted with v
inline vec3 mul3_transposed(const mat4& m, vec3 v) {
  return {m[0][0] * v.x + m[0][1] * v.y + m[0][2] * v.z,
          m[1][0] * v.x + m[1][1] * v.y + m[1][2] * v.z,
          m[2][0] * v.x + m[2][1] * v.y + m[2][2] * v.z};
}
// glm compute_inverse<4,4> (cofactor form)
mat4 inverse(const mat4& m) {
  float Coef00 = m[2][2] * m[3][3] - m[3][2] * m[2][3];
  float Coef02 = m[1][2] * m[3][3] - m[3][2] * m[1][3];
  float Coef03 = m[1][2] * m[2][3] - m[2][2] * m[1][3];
  float Coef04 = m[2][1] * m[3][3] - m[3][1] * m[2][3];
  float Coef06 = m[1][1] * m[3][3] - m[3][1] * m[1][3];
  float Coef07 = m[1][1] * m[2][3] - m[2][1] * m[1][3];
  float Coef08 = m[2][1] * m[3][2] - m[3][1] * m[2][2];
  float Coef10 = m[1][1] * m[3][2] - m[3][1] * m[1][2];
  float Coef11 = m[1][1] * m[2][2] - m[2][1] * m[1][2];
  float Coef12 = m[2][0] * m[3][3] - m[3][0] * m[2][3];
  float Coef14 = m[1][0] * m[3][3] - m[3][0] * m[1][3];
  float Coef15 = m[1][0] * m[2][3] - m[2][0] * m[1][3];
  float Coef16 = m[2][0] * m[3][2] - m[3][0] * m[2][2];
  float Coef18 = m[1][0] * m[3][2] - m[3][0] * m[1][2];
  float Coef19 = m[1][0] * m[2][2] - m[2][0] * m[1][2];
  float Coef20 = m[2][0] * m[3][1] - m[3][0] * m[2][1];
  float Coef22 = m[1][0] * m[3][1] - m[3][0] * m[1][1];
  float Coef23 = m[1][0] * m[2][1] - m[2][0] * m[1][1];
  vec4 Fac0{Coef00, Coef00, Coef02, Coef03};
  vec4 Fac1{Coef04, Coef04, Coef06, Coef07};
  vec4 Fac2{Coef08, Coef08, Coef10, Coef11};
  vec4 Fac3{Coef12, Coef12, Coef14, Coef15};
  vec4 Fac4{Coef16, Coef16, Coef18, Coef19};
  vec4 Fac5{Coef20, Coef20, Coef22, Coef23};
  vec4 Vec0{m[1][0], m[0][0], m[0][0], m[0][0]};
  vec4 Vec1{m[1][1], m[0][1], m[0][1], m[0][1]};
  vec4 Vec2{m[1][2], m[0][2], m[0][2], m[0][2]};
  vec4 Vec3{m[1][3], m[0][3], m[0][3], m[0][3]};
  vec4 Inv0 = (Vec1 * Fac0 - Vec2 * Fac1) + Vec3 * Fac2;
  vec4 Inv1 = (Vec0 * Fac0 - Vec2 * Fac3) + Vec3 * Fac4;
  vec4 Inv2 = (Vec0 * Fac1 - Vec1 * Fac3) + Vec3 * Fac5;
  vec4 Inv3 = (Vec0 * Fac2 - Vec1 * Fac4) + Vec2 * Fac5;
  vec4 SignA{+1, -1, +1, -1};
  vec4 SignB{-1, +1, -1, +1};
  mat4 inv;
  inv[0] = Inv0 * SignA;
  inv[1] = Inv1 * SignB;
  inv[2] = Inv2 * SignA;
  inv[3] = Inv3 * SignB;
  vec4 Row0{inv[0][0], inv[1][0], inv[2][0], inv[3][0]};
  vec4 Dot0 = m[0] * Row0;
  float Dot1 = (Dot0.x + Dot0.y) + (Dot0.z + Dot0.w);
  float OneOverDeterminant = 1.0f / Dot1;
  for (int i = 0; i < 4; i++) inv[i] = inv[i] * OneOverDeterminant;
  return inv;
}

// ----------------------------------------------------------------------------------------------
// RNG: Philox4x32-10 (Salmon et al., SC'11), counter = (a, b, block, tag), key = seed.
inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; r++) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    uint32_t n0 = hi1 ^ c[1] ^ k0, n1 = lo1, n2 = hi0 ^ c[3] ^ k1, n3 = lo0;
    c[0] = n0;
    c[1] = n1;
    c[2] = n2;
    c[3] = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}
constexpr uint32_t kTagPath = 0x52543250u;    // "RT2P"
constexpr uint32_t kTagPerlin = 0x52543254u;  // "RT2T"

struct Rng {
  uint32_t k0, k1, a, b, tag;
  uint32_t block{0};
  uint32_t buf[4]{};
  int idx{4};
  uint64_t draws{0};
  Rng(uint64_t seed, uint32_t a_, uint32_t b_, uint32_t tag_)
      : k0((uint32_t)seed), k1((uint32_t)(seed >> 32)), a(a_), b(b_), tag(tag_) {}
  uint32_t next_u32() {
    if (idx == 4) {
      buf[0] = a;
      buf[1] = b;
      buf[2] = block++;
      buf[3] = tag;
      philox4x32_10(buf, k0, k1);
      idx = 0;
    }
    draws++;
    return buf[idx++];
  }
  // uniform float in [0,1) from the top 24 bits (exact)
  float RandReal() { return (float)(next_u32() >> 8) * (1.0f / 16777216.0f); }
  // Math.hpp:15
  float RandReal(float min, float max) { return min + RandReal() * (max - min); }
  // Math.hpp:18
  int RandInt(int min, int max) { return (int)(RandReal((float)min, (float)(max + 1))); }
};

// Math.hpp:20-43
inline vec3 RandVec3(Rng& g, float min, float max) {
  float x = g.RandReal(min, max);
  float y = g.RandReal(min, max);
  float z = g.RandReal(min, max);
  return {x, y, z};
}
// (cos 2 pi v, sin 2 pi v) for v in [0, 1): quarter turn by the exact split 4v = q + x, then
// degree-9 odd / degree-8 even polynomials in x (max error 2e-7). The kernel evaluates the same
// operations in the same order (render.hip cos_sin_2pi), so both round identically.
// sin(x) of a float (the marble texture, Texture.cpp:16 std::sin): k = rint(x 2/pi), x - k pi/2 by a
// three-part Cody-Waite split in fmas, quarter-turn polynomials in fmas; within 9e-8 of sin for
// |x| <= 5000. |x| >= 2^24 gives x - x. The kernel's sin_f evaluates the same operations in the same
// order (tests/test_oracle_kat.py pins it against sin).
inline float SinF(float x) {
  if (!(std::fabs(x) < 0x1p24f)) return x - x;
  const float k = std::rint(x * 0.636619772f);
  float r = std::fma(-k, 1.57079637f, x);
  r = std::fma(-k, -4.37113883e-08f, r);
  r = std::fma(-k, -1.71512451e-15f, r);
  const float z = r * r;
  const float s = std::fma(std::fma(std::fma(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f), z * r, r);
  const float c = std::fma(std::fma(std::fma(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f),
                           z * z, std::fma(-0.5f, z, 1.0f));
  const int q = (int)(k - 4.0f * std::floor(k * 0.25f));
  const float v = (q & 1) ? c : s;
  return q >= 2 ? -v : v;
}

inline void CosSin2Pi(float v, float& c, float& s) {
  const float t = v * 4.0f;
  const int q = (int)t;
  const float x = t - (float)q;
  const float x2 = x * x;
  // Horner steps as fused multiply-adds (one rounding each; the oracle evaluates the same fmas)
  const float sp = std::fma(std::fma(std::fma(std::fma(1.509560242993757e-4f, x2, -4.672547802329063e-3f), x2, 7.968873530626297e-2f), x2,
                             -6.459634304046631e-1f), x2, 1.570796251296997f) * x;
  const float cp = std::fma(std::fma(std::fma(std::fma(8.59465915709734e-4f, x2, -2.0813362672924995e-2f), x2, 2.536526620388031e-1f), x2,
                             -1.2336987257003784f), x2, 1.0f);
  switch (q) {
    case 0: c = cp; s = sp; break;
    case 1: c = -sp; s = cp; break;
    case 2: c = -cp; s = -sp; break;
    default: c = sp; s = -cp; break;
  }
}
// ln(u) of a 24-bit uniform u in [0, 1) (ConstantMedium.cpp:38 takes std::log(RandReal())): -inf
// at 0, else e ln2 + log1p(f) with u = 2^e (1 + f), 1 + f in [sqrt(1/2), sqrt(2)), log1p by a
// degree-10 polynomial f + f^2 Q(f) (Q of degree 8, max 0.7 ulp over the range) and ln2 split so
// that e ln2_hi is exact; within 1 ulp of ln(u) for every u (tests/test_oracle_kat.py). Float
// operations in a fixed order, fused multiply-adds explicit: the kernel (render.hip log_u) computes
// the same bits. (The reference's glibc logf is itself not correctly rounded; both are within an ulp.)
inline float LogU(float u) {
  if (u == 0.0f) return -INFINITY;
  uint32_t b;
  memcpy(&b, &u, 4);
  int e = (int)(b >> 23) - 127;
  const uint32_t mb = (b & 0x007FFFFFu) | 0x3F800000u;
  float m;
  memcpy(&m, &mb, 4);
  if (m > 1.41421354f) {
    m = m * 0.5f;
    e += 1;
  }
  const float f = m - 1.0f;
  float q = -0.07477458566427231f;
  q = std::fma(q, f, 0.12822002172470093f);
  q = std::fma(q, f, -0.13261467218399048f);
  q = std::fma(q, f, 0.1419624537229538f);
  q = std::fma(q, f, -0.16608606278896332f);
  q = std::fma(q, f, 0.2000119835138321f);
  q = std::fma(q, f, -0.2500157654285431f);
  q = std::fma(q, f, 0.3333333730697632f);
  q = std::fma(q, f, -0.49999988079071045f);
  const float l1p = std::fma(f * f, q, f);
  const float ef = (float)e;
  return std::fma(ef, 0.693145751953125f, std::fma(ef, 1.42860677e-06f, l1p));
}

// Math.hpp:26-43 draw RandUnitVec3 = normalize(RandInUnitSphere()) by rejection in [-1,1]^3 and
// RandInUnitDisk by rejection in [-1,1]^2. The same distributions (uniform on the unit sphere /
// in the unit disk) are drawn here by the inverse-CDF maps, two uniforms each and no retry loop
// (a rejection loop costs a GPU wave its unluckiest lane's retries): z = 1 - 2u, phi = 2 pi v;
// r = sqrt(u), phi = 2 pi v.
inline vec3 RandUnitVec3(Rng& g) {
  if (g_controls & kCtlRefMath) {  // Math.hpp:26-32, 45: normalize(RandInUnitSphere())
    while (true) {
      const float x = g.RandReal(-1, 1), y = g.RandReal(-1, 1), z = g.RandReal(-1, 1);
      const vec3 p{x, y, z};
      const float length_sq = dot(p, p);
      if (1e-160 < (double)length_sq && (double)length_sq <= 1.0) return normalize(p);
    }
  }
  const float u = g.RandReal();
  const float v = g.RandReal();
  const float z = 1.0f - 2.0f * u;
  const float r = std::sqrt(1.0f - z * z);
  float c, s;
  CosSin2Pi(v, c, s);
  return {r * c, r * s, z};
}
inline vec3 RandInUnitDisk(Rng& g) {
  if (g_controls & kCtlRefMath) {
    // Math.hpp:34-41 draws both inside one constructor call, vec3(RandReal(-1, 1), RandReal(-1, 1), 0): the
    // language leaves the order open, and the g++ build of the reference (oracle/_ref) evaluates the
    // arguments right to left, so the first uniform is y (tests/test_reference_build.py pins this)
    while (true) {
      const float y = g.RandReal(-1, 1), x = g.RandReal(-1, 1);
      const vec3 p{x, y, 0.0f};
      if ((double)dot(p, p) < 1.0) return p;
    }
  }
  const float u = g.RandReal();
  const float v = g.RandReal();
  const float r = std::sqrt(u);
  float c, s;
  CosSin2Pi(v, c, s);
  return {r * c, r * s, 0.0f};
}
// Math.hpp:61-73
inline bool NearZero(vec3 v) {
  constexpr double kEpsilon = 1e-8;
  return (std::fabs(v.x) < kEpsilon) && (std::fabs(v.y) < kEpsilon) && (std::fabs(v.z) < kEpsilon);
}
inline vec3 Reflect(vec3 v, vec3 n) { return v - (2 * dot(v, n)) * n; }
inline vec3 Refract(vec3 uv, vec3 n, float etai_over_etat) {
  float cos_theta = (float)std::fmin((double)dot(-uv, n), 1.0);
  vec3 r_out_perp = etai_over_etat * (uv + cos_theta * n);
  vec3 r_out_parallel = -std::sqrt(std::fabs(1.0f - dot(r_out_perp, r_out_perp))) * n;
  return r_out_perp + r_out_parallel;
}

// ----------------------------------------------------------------------------------------------
// Interval / AABB / Ray / HitRecord (Interval.hpp, AABB.hpp, Ray.hpp, HitRecord.hpp)
struct Interval {
  float min{kInfinity}, max{-kInfinity};
  Interval() = default;
  Interval(float a, float b) : min(a), max(b) {}
  Interval(const Interval& a, const Interval& b) : min(std::fmin(a.min, b.min)), max(std::fmax(a.max, b.max)) {}
  float Size() const { return max - min; }
  bool Contains(float x) const { return min <= x && x <= max; }
  bool Surrounds(float x) const { return min < x && x < max; }
  Interval Expand(float delta) const {
    float padding = delta / 2.0f;
    return {min - padding, max + padding};
  }
};
#define kUniverse (Interval{-kInfinity, kInfinity})

struct Ray {
  vec3 origin, direction;
  float time{0};
  vec3 At(float t) const { return origin + direction * t; }
};

struct AABB {
  Interval x, y, z;
  AABB() = default;
  AABB(vec3 a, vec3 b)
      : x(std::fmin(a.x, b.x), std::fmax(a.x, b.x)),
        y(std::fmin(a.y, b.y), std::fmax(a.y, b.y)),
        z(std::fmin(a.z, b.z), std::fmax(a.z, b.z)) {
    Pad();
  }
  AABB(const AABB& a, const AABB& b) : x(a.x, b.x), y(a.y, b.y), z(a.z, b.z) { Pad(); }
  const Interval& Axis(int n) const { return n == 0 ? x : (n == 1 ? y : z); }
  vec3 Min() const { return {x.min, y.min, z.min}; }
  vec3 Max() const { return {x.max, y.max, z.max}; }
  bool Hit(const Ray& r, Interval ray_t) const {
    for (int axis = 0; axis < 3; axis++) {
      const Interval& ax = Axis(axis);
      const float ad_inv = 1.f / r.direction[axis];
      float t0 = (ax.min - r.origin[axis]) * ad_inv;
      float t1 = (ax.max - r.origin[axis]) * ad_inv;
      if (t1 < t0) std::swap(t0, t1);
      ray_t.min = gmax(t0, ray_t.min);
      ray_t.max = gmin(t1, ray_t.max);
      if (ray_t.max <= ray_t.min) return false;
    }
    return true;
  }
  int LongestAxis() const {
    if (x.Size() > y.Size()) return x.Size() > z.Size() ? 0 : 2;
    return y.Size() > z.Size() ? 1 : 2;
  }
  void Pad() {
    constexpr float kDelta = 0.0001f;
    if (x.Size() < kDelta) x = x.Expand(kDelta);
    if (y.Size() < kDelta) y = y.Expand(kDelta);
    if (z.Size() < kDelta) z = z.Expand(kDelta);
  }
};

struct HitRecord {
  vec3 point, normal;
  vec2 uv;
  float t{0};
  int material{-1};
  bool front_face{false};
  void SetFaceNormal(const Ray& r, vec3 outward) {
    front_face = dot(r.direction, outward) < 0;
    normal = ((float)(((int)front_face) << 1) - 1.0f) * outward;
  }
};

struct Counters {
  uint64_t rays{0}, bvh{0}, quad{0}, sphere{0}, xform{0}, medium{0}, list{0};
  void add(const Counters& o) {
    rays += o.rays; bvh += o.bvh; quad += o.quad; sphere += o.sphere; xform += o.xform;
    medium += o.medium; list += o.list;
  }
};

struct Scene;
struct Ctx {
  const Scene* scene;
  Rng* rng;
  Counters* cnt;
};

struct Hittable {
  virtual ~Hittable() = default;
  virtual bool Hit(Ctx& c, const Ray& r, Interval ray_t, HitRecord& rec) const = 0;
  virtual AABB GetAABB() const = 0;
  virtual bool HasMedium() const { return false; }
};
using HPtr = std::shared_ptr<Hittable>;

// HittableList.cpp:8-22
struct HittableList : Hittable {
  std::vector<HPtr> objects;
  AABB aabb;
  void Add(const HPtr& o) {
    objects.push_back(o);
    aabb = AABB(aabb, o->GetAABB());
  }
  bool Hit(Ctx& c, const Ray& r, Interval ray_t, HitRecord& rec) const override {
    c.cnt->list++;
    HitRecord temp;
    bool hit_any = false;
    for (const auto& h : objects) {
      if (h->Hit(c, r, ray_t, temp)) {
        hit_any = true;
        ray_t.max = temp.t;
        rec = temp;
      }
    }
    return hit_any;
  }
  AABB GetAABB() const override { return aabb; }
  bool HasMedium() const override {
    for (auto& o : objects)
      if (o->HasMedium()) return true;
    return false;
  }
};

// Quad.hpp:13-32, Quad.cpp:8-43
struct Quad : Hittable {
  vec3 q, u, v, w, normal;
  float d;
  uint32_t mat;
  AABB aabb;
  Quad(vec3 q_, vec3 u_, vec3 v_, uint32_t m) : q(q_), u(u_), v(v_), mat(m) {
    vec3 n = cross(u, v);
    normal = normalize(n);
    d = dot(normal, q);
    w = n / dot(n, n);
    aabb = AABB(AABB(q, (q + u) + v), AABB(q + u, q + v));
  }
  bool Hit(Ctx& c, const Ray& r, Interval ray_t, HitRecord& rec) const override {
    c.cnt->quad++;
    float n_dot = dot(normal, r.direction);
    if (std::fabs(n_dot) < 1e-8) return false;
    float t = (d - dot(normal, r.origin)) / n_dot;
    if (!ray_t.Contains(t)) return false;
    vec3 p = r.At(t);
    vec3 pv = p - q;
    float alpha = dot(w, cross(pv, v));
    float beta = dot(w, cross(u, pv));
    Interval unit{0, 1};
    if (!unit.Contains(alpha) || !unit.Contains(beta)) return false;
    rec.uv = {alpha, beta};
    rec.t = t;
    rec.point = p;
    rec.material = (int)mat;
    rec.SetFaceNormal(r, normal);
    return true;
  }
  AABB GetAABB() const override { return aabb; }
};

// Quad.hpp:34-50
std::shared_ptr<HittableList> MakeBox(vec3 a, vec3 b, uint32_t m) {
  auto list = std::make_shared<HittableList>();
  vec3 mn{std::fmin(a.x, b.x), std::fmin(a.y, b.y), std::fmin(a.z, b.z)};
  vec3 mx{std::fmax(a.x, b.x), std::fmax(a.y, b.y), std::fmax(a.z, b.z)};
  vec3 dx{mx.x - mn.x, 0, 0}, dy{0, mx.y - mn.y, 0}, dz{0, 0, mx.z - mn.z};
  list->Add(std::make_shared<Quad>(vec3{mn.x, mn.y, mx.z}, dx, dy, m));
  list->Add(std::make_shared<Quad>(vec3{mx.x, mn.y, mx.z}, -dz, dy, m));
  list->Add(std::make_shared<Quad>(vec3{mx.x, mn.y, mn.z}, -dx, dy, m));
  list->Add(std::make_shared<Quad>(vec3{mn.x, mn.y, mn.z}, dz, dy, m));
  list->Add(std::make_shared<Quad>(vec3{mn.x, mx.y, mx.z}, dx, -dz, m));
  list->Add(std::make_shared<Quad>(vec3{mn.x, mn.y, mn.z}, dx, dz, m));
  return list;
}

// Sphere.hpp:21-29 (moving ctor, which the loader always uses), Sphere.cpp:7-43
struct Sphere : Hittable {
  Ray cd;  // center_displacement
  float radius;
  uint32_t mat;
  AABB aabb;
  Sphere(vec3 c0, vec3 disp, float r, uint32_t m) : radius(r), mat(m) {
    cd.origin = c0;
    cd.direction = disp;
    cd.time = 0;
    vec3 c_0 = cd.At(0), c_1 = cd.At(1);
    aabb = AABB(AABB(c_0 - vec3(r), c_0 + vec3(r)), AABB(c_1 - vec3(r), c_1 + vec3(r)));
  }
  static vec2 GetUV(vec3 p) {
    const float pi = 3.14159265358979323846f;
    float theta = std::acos(-p.y);
    float phi = std::atan2(-p.z, p.x) + pi;
    return {phi / (2.f * pi), theta / pi};
  }
  bool Hit(Ctx& c, const Ray& r, Interval ray_t, HitRecord& rec) const override {
    c.cnt->sphere++;
    vec3 center = cd.At(r.time);
    vec3 oc = center - r.origin;
    float a = dot(r.direction, r.direction);
    float h = dot(r.direction, oc);
    float cc = dot(oc, oc) - radius * radius;
    float disc = h * h - a * cc;
    if (disc < 0) return false;
    float sqrtd = std::sqrt(disc);
    float root = (h - sqrtd) / a;
    if (!ray_t.Surrounds(root)) {
      root = (h + sqrtd) / a;
      if (!ray_t.Surrounds(root)) return false;
    }
    rec.t = root;
    rec.point = r.At(rec.t);
    rec.material = (int)mat;
    vec3 outward = (rec.point - center) / radius;
    rec.SetFaceNormal(r, outward);
    rec.uv = GetUV(outward);  // dead output (no texture reads uv), kept for fidelity
    return true;
  }
  AABB GetAABB() const override { return aabb; }
};

// Transform.cpp:13-88
struct Transformed : Hittable {
  mat4 model, inv_model;
  HPtr obj;
  AABB aabb;
  Transformed(HPtr o, const mat4& m) : model(m), obj(std::move(o)) {
    inv_model = inverse(model);
    AABB e = obj->GetAABB();
    vec3 mn = e.Min(), mx = e.Max();
    vec3 corners[8] = {{mn.x, mn.y, mn.z}, {mx.x, mn.y, mn.z}, {mn.x, mx.y, mn.z}, {mx.x, mx.y, mn.z},
                       {mn.x, mn.y, mx.z}, {mx.x, mn.y, mx.z}, {mn.x, mx.y, mx.z}, {mx.x, mx.y, mx.z}};
    vec3 nmin(kInfinity), nmax(-kInfinity);
    for (auto& cn : corners) {
      vec3 t = xyz(mul(model, vec4{cn.x, cn.y, cn.z, 1.f}));
      nmin.x = std::fmin(nmin.x, t.x);
      nmin.y = std::fmin(nmin.y, t.y);
      nmin.z = std::fmin(nmin.z, t.z);
      nmax.x = std::fmax(nmax.x, t.x);
      nmax.y = std::fmax(nmax.y, t.y);
      nmax.z = std::fmax(nmax.z, t.z);
    }
    aabb = AABB(nmin, nmax);
  }
  Ray WorldToModel(const Ray& r) const {
    vec3 o = xyz(mul(inv_model, vec4{r.origin.x, r.origin.y, r.origin.z, 1}));
    vec3 d = mul3(inv_model, r.direction);
    if (!(g_controls & kCtlWorldT)) d = normalize(d);  // Transform.cpp:17: the quirk (model-space t)
    return Ray{o, d, r.time};
  }
  bool Hit(Ctx& c, const Ray& r, Interval ray_t, HitRecord& rec) const override {
    c.cnt->xform++;
    Ray m = WorldToModel(r);
    if (!obj->Hit(c, m, ray_t, rec)) return false;
    rec.point = xyz(mul(model, vec4{rec.point.x, rec.point.y, rec.point.z, 1.f}));
    // normal_mat = mat3(transpose(inverse(model)))
    rec.normal = normalize(mul3_transposed(inv_model, rec.normal));
    return true;
  }
  AABB GetAABB() const override { return aabb; }
  bool HasMedium() const override { return obj->HasMedium(); }
};

// ConstantMedium.cpp:10-58
struct ConstantMedium : Hittable {
  HPtr boundary;
  float neg_inv_density;
  uint32_t mat;
  ConstantMedium(HPtr b, float density, uint32_t m)
      : boundary(std::move(b)), neg_inv_density((float)(-1.0 / (double)density)), mat(m) {}
  bool Hit(Ctx& c, const Ray& r, Interval ray_t, HitRecord& rec) const override {
    c.cnt->medium++;
    HitRecord rec1, rec2;
    if (!boundary->Hit(c, r, kUniverse, rec1)) return false;
    if (!boundary->Hit(c, r, Interval((float)((double)rec1.t + 0.0001), kInfinity), rec2)) return false;
    rec1.t = std::fmax(rec1.t, ray_t.min);
    rec2.t = std::fmin(rec2.t, ray_t.max);
    if (rec1.t >= rec2.t) return false;
    rec1.t = (float)std::fmax((double)rec1.t, 0.0);
    float ray_len = length(r.direction);
    float dist_inside = (rec2.t - rec1.t) * ray_len;
    const float u = c.rng->RandReal();
    float hit_dist = neg_inv_density * ((g_controls & kCtlRefMath) ? std::log(u) : LogU(u));
    if (hit_dist > dist_inside) return false;
    rec.t = rec1.t + hit_dist / ray_len;
    rec.point = r.At(rec.t);
    rec.normal = vec3{1, 0, 0};
    rec.front_face = true;
    rec.material = (int)mat;
    return true;
  }
  AABB GetAABB() const override { return boundary->GetAABB(); }
  bool HasMedium() const override { return true; }
};

// BVH.cpp:10-55
struct BVHNode : Hittable {
  HPtr left, right;
  AABB aabb;
  BVHNode(std::vector<HPtr>& objects, size_t start, size_t end) {
    size_t span = end - start;
    for (size_t i = start; i < end; i++) aabb = AABB(aabb, objects[i]->GetAABB());
    if (span == 1) {
      left = right = objects[start];
    } else if (span == 2) {
      left = objects[start];
      right = objects[start + 1];
    } else {
      int axis = aabb.LongestAxis();
      std::sort(objects.begin() + (long)start, objects.begin() + (long)end,
                [axis](const HPtr& a, const HPtr& b) {
                  return a->GetAABB().Axis(axis).min < b->GetAABB().Axis(axis).min;
                });
      size_t mid = start + span / 2;
      left = std::make_shared<BVHNode>(objects, start, mid);
      right = std::make_shared<BVHNode>(objects, mid, end);
    }
  }
  bool Hit(Ctx& c, const Ray& r, Interval ray_t, HitRecord& rec) const override {
    c.cnt->bvh++;
    if (!(g_controls & kCtlNoSlab) && !aabb.Hit(r, ray_t)) return false;
    bool hit_left = left->Hit(c, r, ray_t, rec);
    if ((g_controls & kCtlSingleLeaf) && left == right) return hit_left;
    bool hit_right = right->Hit(c, r, Interval(ray_t.min, hit_left ? rec.t : ray_t.max), rec);
    return hit_left || hit_right;
  }
  AABB GetAABB() const override { return aabb; }
  bool HasMedium() const override { return left->HasMedium() || right->HasMedium(); }
};

// ----------------------------------------------------------------------------------------------
// Textures / Perlin / Materials (Texture.*, PerlinNoiseGen.cpp, Material.*)
struct Perlin {
  int point_count{256};
  std::vector<vec3> rand_vec3;
  std::vector<int> perm_x, perm_y, perm_z;
  void Init(Rng& g) {
    rand_vec3.resize((size_t)point_count);
    for (int i = 0; i < point_count; i++) rand_vec3[(size_t)i] = normalize(RandVec3(g, -1, 1));
    GenPerm(g, perm_x);
    GenPerm(g, perm_y);
    GenPerm(g, perm_z);
  }
  void GenPerm(Rng& g, std::vector<int>& p) const {
    p.clear();
    for (int i = 0; i < point_count; i++) p.push_back(i);
    for (int i = point_count - 1; i > 0; i--) {
      int target = g.RandInt(0, i);
      std::swap(p[(size_t)i], p[(size_t)target]);
    }
  }
  static float Interp(const vec3 c[2][2][2], float u, float v, float w) {
    float uu = u * u * (3 - 2 * u);
    float vv = v * v * (3 - 2 * v);
    float ww = w * w * (3 - 2 * w);
    float accum = 0;
    for (int i = 0; i < 2; i++)
      for (int j = 0; j < 2; j++)
        for (int k = 0; k < 2; k++) {
          vec3 weight_v{u - (float)i, v - (float)j, w - (float)k};
          accum += ((float)i * uu + (float)(1 - i) * (1 - uu)) * ((float)j * vv + (float)(1 - j) * (1 - vv)) *
                   ((float)k * ww + (float)(1 - k) * (1 - ww)) * dot(c[i][j][k], weight_v);
        }
    return accum;
  }
  float Noise(vec3 p) const {
    float u = p.x - std::floor(p.x);
    float v = p.y - std::floor(p.y);
    float w = p.z - std::floor(p.z);
    int i = (int)std::floor(p.x), j = (int)std::floor(p.y), k = (int)std::floor(p.z);
    vec3 c[2][2][2];
    for (int di = 0; di < 2; di++)
      for (int dj = 0; dj < 2; dj++)
        for (int dk = 0; dk < 2; dk++)
          c[di][dj][dk] = rand_vec3[(size_t)(perm_x[(size_t)((i + di) & 255)] ^ perm_y[(size_t)((j + dj) & 255)] ^
                                             perm_z[(size_t)((k + dk) & 255)])];
    return Interp(c, u, v, w);
  }
  float Turb(vec3 p, int depth = 7) const {
    float accum = 0.f;
    vec3 tp = p;
    float weight = 1.0f;
    for (int i = 0; i < depth; i++) {
      accum += weight * Noise(tp);
      weight = (float)((double)weight * 0.5);
      tp = tp * 2.0f;
    }
    return std::fabs(accum);
  }
};

enum TexType { kSolid = 0, kChecker = 1, kNoise = 2 };
struct Texture {
  int type{kSolid};
  vec3 albedo{1, 1, 1};
  float inv_scale{1};
  uint32_t even{0}, odd{0};
  float scale{1};
  int noise_type{1};  // NoiseType::kMarble
  std::shared_ptr<Perlin> perlin;
};

enum MatType { kMetal = 0, kLambertian = 1, kDielectric = 2, kTextureMat = 3, kDiffuseLight = 4, kIsotropic = 5 };
struct Material {
  int type{kLambertian};
  vec3 albedo{1, 1, 1};
  float fuzz{0};
  float refraction_index{1};
  uint32_t tex_idx{0};
};

struct Camera {
  vec3 center_{0, 0, 0}, lookat_{0, 0, -1}, view_up_{0, 1, 0};
  vec3 viewport_upper_left_, pixel00_loc_, pixel_delta_u_, pixel_delta_v_, defocus_disk_u_, defocus_disk_v_;
  float defocus_angle_{0}, focus_dist_{10}, vfov_{90.f};
  int dims_x{0}, dims_y{0};
  int sqrt_spp{1};
  float recip_sqrt_spp{1};
  int samples_per_pixel{1};
  // Camera.hpp:16-48
  void Update() {
    float theta = radians(vfov_);
    float h = std::tan(theta / 2);
    vec3 w = normalize(center_ - lookat_);
    vec3 u = normalize(cross(view_up_, w));
    vec3 v = cross(w, u);
    float viewport_height = (float)(2.0 * (double)h * (double)focus_dist_);
    float viewport_width = viewport_height * ((float)dims_x / (float)dims_y);
    vec3 lu = viewport_width * u;
    vec3 lv = viewport_height * v;
    pixel_delta_u_ = lu / (float)dims_x;
    pixel_delta_v_ = lv / (float)dims_y;
    viewport_upper_left_ = ((center_ - vec3(w * focus_dist_)) - lu / 2.0f) - lv / 2.0f;
    pixel00_loc_ = viewport_upper_left_ + 0.5f * (pixel_delta_u_ + pixel_delta_v_);
    float defocus_radius = focus_dist_ * std::tan(radians(defocus_angle_ / 2));
    defocus_disk_u_ = u * defocus_radius;
    defocus_disk_v_ = v * defocus_radius;
    sqrt_spp = (int)std::sqrt((double)samples_per_pixel);
    recip_sqrt_spp = (float)(1.0 / (double)sqrt_spp);
  }
  // Camera.hpp:50-67
  Ray GetRay(int x, int y, int s_i, int s_j, Rng& g) const {
    float px = ((float)s_i + g.RandReal()) * recip_sqrt_spp - 0.5f;
    float py = ((float)s_j + g.RandReal()) * recip_sqrt_spp - 0.5f;
    vec3 pixel_center = (pixel00_loc_ + (((float)x + px) * pixel_delta_u_)) + (((float)y + py) * pixel_delta_v_);
    vec3 c = center_;
    if (!(defocus_angle_ <= 0)) {
      vec3 p = RandInUnitDisk(g);
      c = (center_ + (p.x * defocus_disk_u_)) + (p.y * defocus_disk_v_);
    }
    float ray_time = g.RandReal();
    return Ray{c, normalize(pixel_center - c), ray_time};
  }
};

struct Scene {
  HittableList hittable_list;  // after App.cpp:126: a list holding one BVHNode
  std::vector<Material> materials;
  std::vector<Texture> textures;
  Camera cam;
  vec3 background_color{1, 1, 1};
  int dims_x{0}, dims_y{0};
  int n_top_nodes{0};
  std::vector<HPtr> primitives;  // loader "list" (for KATs)
};

vec3 TexValue(const Scene& s, uint32_t idx, vec3 p) {
  const Texture& t = s.textures[idx];
  switch (t.type) {
    case kSolid:
      return t.albedo;
    case kChecker: {
      vec3 sp = t.inv_scale * p;
      int ix = (int)std::floor(sp.x), iy = (int)std::floor(sp.y), iz = (int)std::floor(sp.z);
      return TexValue(s, (ix + iy + iz) % 2 == 0 ? t.even : t.odd, p);
    }
    case kNoise:
      if (t.noise_type == 1) {
        float arg = t.scale * p.z + 10 * t.perlin->Turb(p);
        if (g_controls & kCtlRefMath) return (t.albedo * 0.5f) * (1 + std::sin(arg));  // sinf (Texture.cpp:16)
        return (t.albedo * 0.5f) * (1 + SinF(arg));
      }
      return (t.albedo * 0.5f) * (1.0f + t.perlin->Noise(t.scale * p));
  }
  return {};
}

// Material.cpp:10-83. Returns is_scattered; attenuation/scattered out; emission separately.
bool Scatter(const Scene& s, Rng& g, const Ray& r_in, const HitRecord& rec, vec3& att, Ray& scattered) {
  const Material& m = s.materials[(size_t)rec.material];
  switch (m.type) {
    case kMetal: {
      vec3 reflected = normalize(Reflect(r_in.direction, rec.normal)) + (m.fuzz * RandUnitVec3(g));
      scattered = Ray{rec.point, reflected, r_in.time};
      att = m.albedo;
      return true;
    }
    case kDielectric: {
      att = vec3(1.0f);
      float ri = rec.front_face ? (float)(1.0 / (double)m.refraction_index) : m.refraction_index;
      vec3 unit_dir = normalize(r_in.direction);
      float cos_theta = gmin(dot(-unit_dir, rec.normal), 1.0f);
      float sin_theta = std::sqrt(1.f - cos_theta * cos_theta);
      bool cannot_refract = ri * sin_theta > 1.0;
      bool reflect = cannot_refract;
      if (!reflect) {
        float r0 = (1 - ri) / (1 + ri);
        r0 = r0 * r0;
        double x = (double)(1 - cos_theta);
        double x2 = x * x;
        double x5 = (x2 * x2) * x;
        if (g_controls & kCtlRefMath) x5 = std::pow((double)(1 - cos_theta), 5);  // Material.cpp:24
        double schlick = (double)r0 + (double)(1 - r0) * x5;
        reflect = schlick > (double)g.RandReal();
      }
      vec3 dir = reflect ? Reflect(unit_dir, rec.normal) : Refract(unit_dir, rec.normal, ri);
      scattered = Ray{rec.point, dir, r_in.time};
      return true;
    }
    case kLambertian:
    case kTextureMat: {
      vec3 dir = rec.normal + RandUnitVec3(g);
      if (NearZero(dir)) dir = rec.normal;
      scattered = Ray{rec.point, dir, r_in.time};
      att = m.type == kLambertian ? m.albedo : TexValue(s, m.tex_idx, rec.point);
      return true;
    }
    case kIsotropic: {
      scattered = Ray{rec.point, RandUnitVec3(g), r_in.time};
      att = TexValue(s, m.tex_idx, rec.point);
      return true;
    }
    default:  // DiffuseLight
      return false;
  }
}

vec3 Emit(const Scene& s, const HitRecord& rec) {
  const Material& m = s.materials[(size_t)rec.material];
  if (m.type == kDiffuseLight) return TexValue(s, m.tex_idx, rec.point);
  return vec3{0, 0, 0};
}

// RayTracer.cpp:20-45 (recursive form, faithful product order)
vec3 RayColor(Ctx& c, const Ray& r, int depth) {
  if (depth <= 0) return {0, 0, 0};
  c.cnt->rays++;
  HitRecord rec;
  if (!c.scene->hittable_list.Hit(c, r, Interval((float)0.001, kInfinity), rec)) return c.scene->background_color;
  Ray scattered;
  vec3 att;
  vec3 emission = Emit(*c.scene, rec);
  if (Scatter(*c.scene, *c.rng, r, rec, att, scattered)) return att * RayColor(c, scattered, depth - 1) + emission;
  return emission;
}

// Same path, throughput accumulated front-to-back (the order a single-pass GPU kernel uses).
// Identical RNG draws and geometry; differs from RayColor only in the rounding of the product
// of attenuations (non-light materials emit exactly 0).
vec3 RayColorForward(Ctx& c, Ray r, int depth) {
  vec3 thr{1, 1, 1};
  while (true) {
    if (depth <= 0) return {0, 0, 0};
    c.cnt->rays++;
    HitRecord rec;
    if (!c.scene->hittable_list.Hit(c, r, Interval((float)0.001, kInfinity), rec))
      return thr * c.scene->background_color;
    Ray scattered;
    vec3 att;
    vec3 emission = Emit(*c.scene, rec);
    if (!Scatter(*c.scene, *c.rng, r, rec, att, scattered)) return thr * emission;
    thr = thr * att;
    r = scattered;
    depth--;
  }
}

// ----------------------------------------------------------------------------------------------
// Minimal JSON (nlohmann::json-compatible subset for the scene schema).
struct J {
  enum T { Null, Bool, Num, Str, Arr, Obj } t{Null};
  double num{0};
  bool b{false};
  std::string s;
  std::vector<J> arr;
  std::vector<std::pair<std::string, J>> obj;
  const J* find(const char* k) const {
    if (t != Obj) return nullptr;
    for (auto& kv : obj)
      if (kv.first == k) return &kv.second;
    return nullptr;
  }
  bool contains(const char* k) const { return find(k) != nullptr; }
};
struct JParser {
  const char* p;
  const char* e;
  std::string err;
  void ws() {
    while (p < e && (*p == ' ' || *p == '\n' || *p == '\r' || *p == '\t')) p++;
  }
  bool parse(J& out) {
    ws();
    if (p >= e) return fail("unexpected end");
    char c = *p;
    if (c == '{') {
      p++;
      out.t = J::Obj;
      ws();
      if (p < e && *p == '}') return ++p, true;
      while (true) {
        ws();
        J key;
        if (p >= e || *p != '"' || !parse(key)) return fail("expected key");
        ws();
        if (p >= e || *p != ':') return fail("expected ':'");
        p++;
        J val;
        if (!parse(val)) return false;
        out.obj.emplace_back(key.s, std::move(val));
        ws();
        if (p < e && *p == ',') { p++; continue; }
        if (p < e && *p == '}') { p++; return true; }
        return fail("expected ',' or '}'");
      }
    }
    if (c == '[') {
      p++;
      out.t = J::Arr;
      ws();
      if (p < e && *p == ']') return ++p, true;
      while (true) {
        J val;
        if (!parse(val)) return false;
        out.arr.push_back(std::move(val));
        ws();
        if (p < e && *p == ',') { p++; continue; }
        if (p < e && *p == ']') { p++; return true; }
        return fail("expected ',' or ']'");
      }
    }
    if (c == '"') {
      p++;
      out.t = J::Str;
      while (p < e && *p != '"') {
        if (*p == '\\' && p + 1 < e) { p++; out.s.push_back(*p == 'n' ? '\n' : *p); p++; continue; }
        out.s.push_back(*p++);
      }
      if (p >= e) return fail("unterminated string");
      p++;
      return true;
    }
    if (!strncmp(p, "true", 4)) { out.t = J::Bool; out.b = true; p += 4; return true; }
    if (!strncmp(p, "false", 5)) { out.t = J::Bool; out.b = false; p += 5; return true; }
    if (!strncmp(p, "null", 4)) { out.t = J::Null; p += 4; return true; }
    char* end = nullptr;
    out.num = strtod(p, &end);
    if (end == p) return fail("bad value");
    out.t = J::Num;
    p = end;
    return true;
  }
  bool fail(const char* m) {
    if (err.empty()) err = m;
    return false;
  }
};

// nlohmann value(key, default) helpers
double jnum(const J& o, const char* k, double d) {
  const J* v = o.find(k);
  return (v && v->t == J::Num) ? v->num : (v && v->t == J::Bool ? (double)v->b : d);
}
int jint(const J& o, const char* k, int d) {
  const J* v = o.find(k);
  return (v && v->t == J::Num) ? (int)v->num : d;
}
float jflt(const J& o, const char* k, float d) {
  const J* v = o.find(k);
  return (v && v->t == J::Num) ? (float)v->num : d;
}
vec3 jvec3(const J& o, const char* k, vec3 d) {
  const J* v = o.find(k);
  if (!v || v->t != J::Arr || v->arr.size() < 3) return d;
  return {(float)v->arr[0].num, (float)v->arr[1].num, (float)v->arr[2].num};
}

bool read_json(const std::string& path, J& out, std::string& err) {
  std::ifstream f(path, std::ios::binary);
  if (!f) {
    err = "cannot open " + path;
    return false;
  }
  std::stringstream ss;
  ss << f.rdbuf();
  std::string txt = ss.str();
  JParser jp{txt.data(), txt.data() + txt.size(), {}};
  if (!jp.parse(out)) {
    err = "json parse error in " + path + ": " + jp.err;
    return false;
  }
  return true;
}

// Serialize.cpp:32-38 (LoadCamera)
Camera LoadCamera(const J& o) {
  Camera cam;
  cam.vfov_ = (float)jint(o, "fov", 90);
  cam.center_ = jvec3(o, "center", {0, 0, 1});
  cam.lookat_ = jvec3(o, "look_at", {0, 0, 0});
  cam.defocus_angle_ = jflt(o, "defocus_angle", 0.0f);
  cam.focus_dist_ = jflt(o, "focus_distance", 1.f);
  return cam;
}

mat4 ParseTransform(const J& tj) {
  vec3 tr = jvec3(tj, "translation", {0, 0, 0});
  float qw = 1, qx = 0, qy = 0, qz = 0;  // identity when "rotation" is absent (see header)
  if (const J* r = tj.find("rotation")) {
    if (r->t == J::Arr && r->arr.size() >= 4) {
      float angle = radians((float)r->arr[0].num);
      vec3 axis{(float)r->arr[1].num, (float)r->arr[2].num, (float)r->arr[3].num};
      float s = std::sin(angle * 0.5f);
      qw = std::cos(angle * 0.5f);
      qx = axis.x * s;
      qy = axis.y * s;
      qz = axis.z * s;
    }
  }
  vec3 sc = jvec3(tj, "scale", {1, 1, 1});
  mat4 T = mat4::identity();
  T[3] = vec4{tr.x, tr.y, tr.z, 1};
  // glm mat3_cast
  float qxx = qx * qx, qyy = qy * qy, qzz = qz * qz, qxz = qx * qz, qxy = qx * qy, qyz = qy * qz;
  float qwx = qw * qx, qwy = qw * qy, qwz = qw * qz;
  mat4 R = mat4::identity();
  R[0][0] = 1.f - 2.f * (qyy + qzz);
  R[0][1] = 2.f * (qxy + qwz);
  R[0][2] = 2.f * (qxz - qwy);
  R[1][0] = 2.f * (qxy - qwz);
  R[1][1] = 1.f - 2.f * (qxx + qzz);
  R[1][2] = 2.f * (qyz + qwx);
  R[2][0] = 2.f * (qxz + qwy);
  R[2][1] = 2.f * (qyz - qwx);
  R[2][2] = 1.f - 2.f * (qxx + qyy);
  mat4 S = mat4::identity();
  S[0][0] = sc.x;
  S[1][1] = sc.y;
  S[2][2] = sc.z;
  return mul(mul(T, R), S);
}

// Serialize.cpp:161-197 (ParseNode)
HPtr ParseNode(const std::vector<HPtr>& list, const J& node, std::string& err) {
  HPtr ret;
  if (node.contains("primitive")) {
    int idx = jint(node, "primitive", -1);
    if (idx < 0 || idx >= (int)list.size()) {
      err = "primitive index out of range";
      return nullptr;
    }
    ret = list[(size_t)idx];
  }
  if (const J* ch = node.find("children")) {
    if (ch->t != J::Arr) {
      err = "children entry must be an array";
      return nullptr;
    }
    auto cl = std::make_shared<HittableList>();
    if (ret) cl->Add(ret);
    for (auto& c : ch->arr) {
      HPtr h = ParseNode(list, c, err);
      if (!h) return nullptr;
      cl->Add(h);
    }
    ret = cl;
  }
  if (!ret) {
    err = "error parsing node";
    return nullptr;
  }
  if (const J* tj = node.find("transform")) {
    if (tj->t == J::Obj) return std::make_shared<Transformed>(ret, ParseTransform(*tj));
  }
  return ret;
}

// Serialize.cpp:199-360 (LoadScene) + the documented legacy-schema adapter
Scene* LoadScene(const std::string& path, uint64_t seed, std::string& err) {
  J obj;
  if (!read_json(path, obj, err)) return nullptr;
  auto sc = std::make_unique<Scene>();
  std::string dir = path.substr(0, path.find_last_of('/') + 1);
  sc->background_color = jvec3(obj, "background_color", {1, 1, 1});
  const J* cam = obj.find("camera");
  if (cam && cam->t == J::Obj) {
    sc->cam = LoadCamera(*cam);
  } else {
    std::string name = (cam && cam->t == J::Str) ? cam->s : std::string("cam1");  // legacy adapter
    J cj;
    if (!read_json(dir + name + ".json", cj, err)) return nullptr;
    sc->cam = LoadCamera(cj);
  }
  uint32_t noise_ordinal = 0;
  if (const J* tx = obj.find("textures")) {
    if (tx->t == J::Arr) {
      for (auto& t : tx->arr) {
        Texture tex;
        const J* ty = t.find("type");
        std::string type = ty && ty->t == J::Str ? ty->s : "";
        if (type == "solid_color") {
          tex.type = kSolid;
          tex.albedo = jvec3(t, "albedo", {1, 1, 1});
        } else if (type == "checker") {
          tex.type = kChecker;
          tex.inv_scale = 1.f / jflt(t, "scale", 1.0f);
          tex.even = (uint32_t)jint(t, "even_tex_idx", 0);
          tex.odd = (uint32_t)jint(t, "odd_tex_idx", 0);
        } else if (type == "noise") {
          tex.type = kNoise;
          tex.perlin = std::make_shared<Perlin>();
          tex.perlin->point_count = jint(t, "point_count", 256);
          Rng g(seed, noise_ordinal++, 0xFFFFFFFFu, kTagPerlin);
          tex.perlin->Init(g);
          tex.albedo = jvec3(t, "albedo", {1, 1, 1});
          tex.scale = jflt(t, "scale", 1.0f);
          tex.noise_type = jint(t, "noise_type", 1);
        } else {
          err = "Invalid texture type: " + type;
          return nullptr;
        }
        sc->textures.push_back(tex);
      }
    }
  }
  if (const J* mj = obj.find("materials")) {
    for (auto& m : mj->arr) {
      const J* ty = m.find("type");
      std::string type = ty && ty->t == J::Str ? ty->s : "";
      if (type.empty()) {
        err = "material type field empty";
        return nullptr;
      }
      Material mat;
      if (type == "lambertian") {
        mat.type = kLambertian;
        mat.albedo = jvec3(m, "albedo", {1, 1, 1});
      } else if (type == "dielectric") {
        mat.type = kDielectric;
        mat.refraction_index = jflt(m, "refraction_index", 1.0f);
      } else if (type == "metal") {
        mat.type = kMetal;
        mat.albedo = jvec3(m, "albedo", {1, 1, 1});
        mat.fuzz = jflt(m, "fuzz", 0.0f);
      } else if (type == "texture" || type == "diffuse_light") {
        mat.type = type == "texture" ? kTextureMat : kDiffuseLight;
        if (m.contains("tex_idx")) {
          mat.tex_idx = (uint32_t)jint(m, "tex_idx", 0);
        } else if (m.contains("albedo")) {
          mat.tex_idx = (uint32_t)sc->textures.size();
          Texture t;
          t.albedo = jvec3(m, "albedo", {1, 1, 1});
          sc->textures.push_back(t);
        } else {
          err = "invalid " + type + ", must contain tex_idx or albedo";
          return nullptr;
        }
      } else {
        err = "Invalid material type";
        return nullptr;
      }
      sc->materials.push_back(mat);
    }
  }
  std::vector<HPtr>& list = sc->primitives;
  const J* prims = obj.find("primitives");
  bool legacy = prims && prims->t == J::Obj;
  std::vector<HPtr> top;
  if (legacy) {
    // Legacy schema ({"spheres":[{center,radius,material_id,displacement?}], "quads":[{q,u,v,
    // material_id}], "boxes":[{a,b,material_id}]}): one scene node per primitive, the groups in file
    // order, each in array order (build decision, SURVEY.md Finding 3).
    for (auto& grp : prims->obj) {
      for (auto& s : grp.second.arr) {
        const uint32_t mat = (uint32_t)jint(s, "material_id", 0);
        HPtr h;
        if (grp.first == "spheres") {
          h = std::make_shared<Sphere>(jvec3(s, "center", {0, 0, 0}), jvec3(s, "displacement", {0, 0, 0}),
                                       (float)jnum(s, "radius", 0.5), mat);
        } else if (grp.first == "quads") {
          h = std::make_shared<Quad>(jvec3(s, "q", {0, 0, 0}), jvec3(s, "u", {1, 0, 0}), jvec3(s, "v", {0, 0, 1}), mat);
        } else if (grp.first == "boxes") {
          h = MakeBox(jvec3(s, "a", {0, 0, 0}), jvec3(s, "b", {1, 1, 1}), mat);
        } else {
          err = "legacy primitives: unknown group " + grp.first;
          return nullptr;
        }
        list.push_back(h);
        top.push_back(h);
      }
    }
  } else if (prims && prims->t == J::Arr) {
    for (auto& p : prims->arr) {
      const J* ty = p.find("type");
      std::string type = ty && ty->t == J::Str ? ty->s : "";
      HPtr h;
      uint32_t mat = (uint32_t)jint(p, "material", 0);
      if (type == "quad") {
        h = std::make_shared<Quad>(jvec3(p, "q", {0, 0, 0}), jvec3(p, "u", {1, 0, 0}), jvec3(p, "v", {0, 0, 1}), mat);
      } else if (type == "box") {
        h = MakeBox(jvec3(p, "a", {0, 0, 0}), jvec3(p, "b", {1, 1, 1}), mat);
      } else if (type == "sphere") {
        h = std::make_shared<Sphere>(jvec3(p, "center", {0, 0, 0}), jvec3(p, "displacement", {0, 0, 0}),
                                     (float)jnum(p, "radius", 0.5), mat);
      } else {
        continue;  // PrintSceneError("invalid primitive type"); continue;
      }
      if (const J* cm = p.find("constant_medium")) {
        uint32_t midx;
        if (cm->contains("albedo")) {
          Material iso;
          iso.type = kIsotropic;
          iso.tex_idx = (uint32_t)sc->textures.size();
          Texture t;
          t.albedo = jvec3(*cm, "albedo", {0, 0, 0});
          sc->textures.push_back(t);
          midx = (uint32_t)sc->materials.size();
          sc->materials.push_back(iso);
        } else if (cm->contains("material")) {
          midx = (uint32_t)jint(*cm, "material", 0);
        } else {
          continue;
        }
        float density = (float)jnum(*cm, "density", 0.01);
        h = std::make_shared<ConstantMedium>(h, density, midx);
      }
      list.push_back(h);
    }
    if (const J* nodes = obj.find("scene")) {
      for (auto& n : nodes->arr) {
        HPtr h = ParseNode(list, n, err);
        if (!h) return nullptr;
        top.push_back(h);
      }
    }
  }
  for (auto& h : top) {
    // validate material / texture indices (the reference would read out of bounds)
    (void)h;
  }
  if (top.empty()) {
    err = "scene has no objects";
    return nullptr;
  }
  sc->n_top_nodes = (int)top.size();
  if (cam && cam->t == J::Obj) {
    int width = jint(*cam, "width", 0);
    float aspect = jflt(*cam, "aspect_ratio", 0.0f);
    if (width != 0 && aspect != 0.0f) {
      float height = (float)width / aspect;
      sc->dims_x = width;
      sc->dims_y = (int)height;
    }
  }
  // App.cpp:126: wrap the top-level list in one BVHNode
  std::vector<HPtr> objs = top;
  sc->hittable_list.Add(std::make_shared<BVHNode>(objs, 0, objs.size()));
  for (auto& m : sc->materials) {
    if ((m.type == kTextureMat || m.type == kDiffuseLight || m.type == kIsotropic) && m.tex_idx >= sc->textures.size()) {
      err = "material texture index out of range";
      return nullptr;
    }
  }
  return sc.release();
}

}  // namespace oracle

// ================================================================================================
// C entry points (ctypes) — test infrastructure only.
using namespace oracle;

extern "C" {

struct oracle_counters {
  uint64_t rays, bvh, quad, sphere, xform, medium, list, rng_draws;
};

struct oracle_scene_info {
  int dims_x, dims_y;
  int n_materials, n_textures, n_primitives, n_top_nodes;
  float background[3];
  float cam_center[3], cam_lookat[3], cam_vfov, cam_defocus_angle, cam_focus_dist;
};

static thread_local std::string g_err;

const char* oracle_last_error() { return g_err.c_str(); }

// Test controls (see g_controls); set before loading a scene (AABB defaults use kInfinity).
void oracle_set_controls(int mask) { g_controls = mask; }
int oracle_get_controls() { return g_controls; }

void* oracle_scene_load(const char* path, uint64_t seed) {
  std::string err;
  Scene* s = LoadScene(path, seed, err);
  if (!s) g_err = err;
  return s;
}

void oracle_scene_free(void* s) { delete (Scene*)s; }

int oracle_scene_get_info(void* sp, oracle_scene_info* out) {
  Scene* s = (Scene*)sp;
  out->dims_x = s->dims_x;
  out->dims_y = s->dims_y;
  out->n_materials = (int)s->materials.size();
  out->n_textures = (int)s->textures.size();
  out->n_primitives = (int)s->primitives.size();
  out->n_top_nodes = s->n_top_nodes;
  out->background[0] = s->background_color.x;
  out->background[1] = s->background_color.y;
  out->background[2] = s->background_color.z;
  out->cam_center[0] = s->cam.center_.x;
  out->cam_center[1] = s->cam.center_.y;
  out->cam_center[2] = s->cam.center_.z;
  out->cam_lookat[0] = s->cam.lookat_.x;
  out->cam_lookat[1] = s->cam.lookat_.y;
  out->cam_lookat[2] = s->cam.lookat_.z;
  out->cam_vfov = s->cam.vfov_;
  out->cam_defocus_angle = s->cam.defocus_angle_;
  out->cam_focus_dist = s->cam.focus_dist_;
  return 0;
}

// materials as rows of 8 floats: type, albedo.xyz, fuzz, refraction_index, tex_idx, 0
int oracle_scene_materials(void* sp, float* out, int cap) {
  Scene* s = (Scene*)sp;
  int n = (int)s->materials.size();
  for (int i = 0; i < n && i < cap; i++) {
    const Material& m = s->materials[(size_t)i];
    float* r = out + 8 * i;
    r[0] = (float)m.type; r[1] = m.albedo.x; r[2] = m.albedo.y; r[3] = m.albedo.z;
    r[4] = m.fuzz; r[5] = m.refraction_index; r[6] = (float)m.tex_idx; r[7] = 0;
  }
  return n;
}

// textures as rows of 8 floats: type, albedo.xyz, inv_scale|scale, even, odd, noise_type
int oracle_scene_textures(void* sp, float* out, int cap) {
  Scene* s = (Scene*)sp;
  int n = (int)s->textures.size();
  for (int i = 0; i < n && i < cap; i++) {
    const Texture& t = s->textures[(size_t)i];
    float* r = out + 8 * i;
    r[0] = (float)t.type; r[1] = t.albedo.x; r[2] = t.albedo.y; r[3] = t.albedo.z;
    r[4] = t.type == kChecker ? t.inv_scale : t.scale; r[5] = (float)t.even; r[6] = (float)t.odd;
    r[7] = (float)t.noise_type;
  }
  return n;
}

// Perlin tables of noise texture `tex`: vec (pc*3 floats), perm (3*pc ints). Returns point_count.
int oracle_scene_perlin(void* sp, int tex, float* vec, int* perm) {
  Scene* s = (Scene*)sp;
  const Texture& t = s->textures[(size_t)tex];
  if (t.type != kNoise) return -1;
  int pc = t.perlin->point_count;
  for (int i = 0; i < pc; i++) {
    vec[3 * i] = t.perlin->rand_vec3[(size_t)i].x;
    vec[3 * i + 1] = t.perlin->rand_vec3[(size_t)i].y;
    vec[3 * i + 2] = t.perlin->rand_vec3[(size_t)i].z;
    perm[i] = t.perlin->perm_x[(size_t)i];
    perm[pc + i] = t.perlin->perm_y[(size_t)i];
    perm[2 * pc + i] = t.perlin->perm_z[(size_t)i];
  }
  return pc;
}

// Value of texture `tex` (Texture.cpp:7-22) at n points (3 floats in, 3 floats out each).
int oracle_texture_value(void* sp, int tex, const float* points, int n, float* out) {
  Scene* s = (Scene*)sp;
  if (tex < 0 || (size_t)tex >= s->textures.size()) return -1;
  for (int i = 0; i < n; i++) {
    vec3 v = TexValue(*s, (uint32_t)tex, vec3{points[3 * i], points[3 * i + 1], points[3 * i + 2]});
    out[3 * i] = v.x;
    out[3 * i + 1] = v.y;
    out[3 * i + 2] = v.z;
  }
  return 0;
}

// Camera setters (Camera.hpp:69-101) on the scene camera the next renders use:
// in = center(3) look_at(3) view_up(3) vfov defocus_angle focus_distance
void oracle_scene_set_camera(void* sp, const float* in) {
  Scene* s = (Scene*)sp;
  s->cam.center_ = {in[0], in[1], in[2]};
  s->cam.lookat_ = {in[3], in[4], in[5]};
  s->cam.view_up_ = {in[6], in[7], in[8]};
  s->cam.vfov_ = in[9];
  s->cam.defocus_angle_ = in[10];
  s->cam.focus_dist_ = in[11];
}

// Camera basis after Camera::Update for the given dims/spp: 6 vec3 (pixel00, du, dv, center,
// defocus_u, defocus_v) + defocus_angle, recip_sqrt_spp, sqrt_spp.
int oracle_camera_params(void* sp, int w, int h, int spp, float* out) {
  Scene* s = (Scene*)sp;
  Camera c = s->cam;
  c.dims_x = w;
  c.dims_y = h;
  c.samples_per_pixel = spp;
  c.Update();
  vec3 v[6] = {c.pixel00_loc_, c.pixel_delta_u_, c.pixel_delta_v_, c.center_, c.defocus_disk_u_, c.defocus_disk_v_};
  for (int i = 0; i < 6; i++) {
    out[3 * i] = v[i].x;
    out[3 * i + 1] = v[i].y;
    out[3 * i + 2] = v[i].z;
  }
  out[18] = c.defocus_angle_;
  out[19] = c.recip_sqrt_spp;
  out[20] = (float)c.sqrt_spp;
  return 0;
}

// Closest-hit query against the scene (world space). out: hit, t, point.xyz, normal.xyz,
// front, material. Uses a throwaway RNG stream (only media draw).
int oracle_scene_hit(void* sp, const float* o, const float* d, float time, float tmin, float tmax, uint64_t seed,
                     float* out) {
  Scene* s = (Scene*)sp;
  Rng g(seed, 0xFFFFFFF0u, 0, kTagPath);
  Counters cnt;
  Ctx c{s, &g, &cnt};
  Ray r{{o[0], o[1], o[2]}, {d[0], d[1], d[2]}, time};
  HitRecord rec;
  bool hit = s->hittable_list.Hit(c, r, Interval(tmin, tmax), rec);
  out[0] = hit ? 1.f : 0.f;
  out[1] = rec.t;
  out[2] = rec.point.x; out[3] = rec.point.y; out[4] = rec.point.z;
  out[5] = rec.normal.x; out[6] = rec.normal.y; out[7] = rec.normal.z;
  out[8] = rec.front_face ? 1.f : 0.f;
  out[9] = (float)rec.material;
  return hit ? 1 : 0;
}

// Known-answer helpers ----------------------------------------------------------------------
void oracle_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
  uint32_t c[4] = {ctr[0], ctr[1], ctr[2], ctr[3]};
  philox4x32_10(c, key[0], key[1]);
  memcpy(out, c, sizeof(c));
}

// Draw n uniforms from the path stream of (seed, pixel, frame).
void oracle_uniforms(uint64_t seed, uint32_t pixel, uint32_t frame, int n, float* out) {
  Rng g(seed, pixel, frame, kTagPath);
  for (int i = 0; i < n; i++) out[i] = g.RandReal();
}

// n draws of RandUnitVec3 (which = 0) or RandInUnitDisk (which = 1) from the path stream of
// (seed, pixel, frame), 3 floats each; which = 2: CosSin2Pi of the n uniforms in `in` (2 floats each);
// which = 3: LogU of the n values in `in` (1 float each); which = 4: SinF of them
void oracle_samples(int which, uint64_t seed, uint32_t pixel, uint32_t frame, int n, const float* in, float* out) {
  Rng g(seed, pixel, frame, kTagPath);
  for (int i = 0; i < n; i++) {
    if (which == 2) {
      CosSin2Pi(in[i], out[2 * i], out[2 * i + 1]);
      continue;
    }
    if (which == 3) {
      out[i] = LogU(in[i]);
      continue;
    }
    if (which == 4) {
      out[i] = SinF(in[i]);
      continue;
    }
    vec3 v = which == 0 ? RandUnitVec3(g) : RandInUnitDisk(g);
    out[3 * i] = v.x;
    out[3 * i + 1] = v.y;
    out[3 * i + 2] = v.z;
  }
}

// Build a quad and intersect: in = q(3) u(3) v(3) o(3) d(3) tmin tmax ; out = hit t p(3) n(3) front alpha beta
int oracle_quad_hit(const float* in, float* out) {
  Quad q({in[0], in[1], in[2]}, {in[3], in[4], in[5]}, {in[6], in[7], in[8]}, 0);
  Counters cnt;
  Ctx c{nullptr, nullptr, &cnt};
  Ray r{{in[9], in[10], in[11]}, {in[12], in[13], in[14]}, 0};
  HitRecord rec;
  bool h = q.Hit(c, r, Interval(in[15], in[16]), rec);
  out[0] = h; out[1] = rec.t;
  out[2] = rec.point.x; out[3] = rec.point.y; out[4] = rec.point.z;
  out[5] = rec.normal.x; out[6] = rec.normal.y; out[7] = rec.normal.z;
  out[8] = rec.front_face; out[9] = rec.uv.x; out[10] = rec.uv.y;
  return h;
}

// in = center(3) disp(3) radius o(3) d(3) time tmin tmax ; out = hit t p(3) n(3) front
int oracle_sphere_hit(const float* in, float* out) {
  Sphere s({in[0], in[1], in[2]}, {in[3], in[4], in[5]}, in[6], 0);
  Counters cnt;
  Ctx c{nullptr, nullptr, &cnt};
  Ray r{{in[7], in[8], in[9]}, {in[10], in[11], in[12]}, in[13]};
  HitRecord rec;
  bool h = s.Hit(c, r, Interval(in[14], in[15]), rec);
  out[0] = h; out[1] = rec.t;
  out[2] = rec.point.x; out[3] = rec.point.y; out[4] = rec.point.z;
  out[5] = rec.normal.x; out[6] = rec.normal.y; out[7] = rec.normal.z;
  out[8] = rec.front_face;
  return h;
}

// in = min(3) max(3) o(3) d(3) tmin tmax
int oracle_aabb_hit(const float* in) {
  AABB b;
  b.x = Interval(in[0], in[3]);
  b.y = Interval(in[1], in[4]);
  b.z = Interval(in[2], in[5]);
  Ray r{{in[6], in[7], in[8]}, {in[9], in[10], in[11]}, 0};
  return b.Hit(r, Interval(in[12], in[13])) ? 1 : 0;
}

// transform = translation(3), rotation(angle, axis3), scale(3) -> model (16, column-major), inverse (16)
void oracle_transform(const float* in, float* model, float* inv) {
  J tj;
  tj.t = J::Obj;
  auto arr = [](std::initializer_list<float> v) {
    J a;
    a.t = J::Arr;
    for (float x : v) {
      J n;
      n.t = J::Num;
      n.num = x;
      a.arr.push_back(n);
    }
    return a;
  };
  tj.obj.emplace_back("translation", arr({in[0], in[1], in[2]}));
  tj.obj.emplace_back("rotation", arr({in[3], in[4], in[5], in[6]}));
  tj.obj.emplace_back("scale", arr({in[7], in[8], in[9]}));
  mat4 m = ParseTransform(tj);
  mat4 iv = inverse(m);
  for (int c = 0; c < 4; c++)
    for (int r = 0; r < 4; r++) {
      model[4 * c + r] = m[c][r];
      inv[4 * c + r] = iv[c][r];
    }
}

// Render frames [frame_begin, frame_begin + n_frames) of the scene at W x H (OnResize dims) with
// the camera's samples_per_pixel = spp (sets the stratification), accumulating into `accum`
// (float3 per pixel, rank-local compact rows: the rows y whose band b = y / band_h has
// (b % world + b / world) % world == rank, in increasing y). ray_counts (nullable) += rays/pixel.
// forward != 0 selects RayColorForward (GPU product order).
int oracle_render(void* sp, int W, int H, int spp, int max_depth, uint64_t seed, int frame_begin, int n_frames,
                  int band_h, int rank, int world, float* accum, uint32_t* ray_counts, int threads, int forward,
                  oracle_counters* out_cnt) {
  Scene* s = (Scene*)sp;
  Camera cam = s->cam;
  cam.dims_x = W;
  cam.dims_y = H;
  cam.samples_per_pixel = spp;
  cam.Update();
  const int sq = cam.sqrt_spp;
  if (band_h <= 0) band_h = H;
  if (world <= 0) world = 1;
  // rank-local rows
  std::vector<int> rows;
  for (int y = 0; y < H; y++)
    if ((y / band_h % world + y / band_h / world) % world == rank) rows.push_back(y);  // BandRank
  if (threads <= 0) threads = (int)std::max(1u, std::thread::hardware_concurrency());
  std::atomic<size_t> next{0};
  std::vector<Counters> cnts((size_t)threads);
  std::vector<uint64_t> draws((size_t)threads, 0);
  auto work = [&](int tid) {
    Counters& cnt = cnts[(size_t)tid];
    while (true) {
      size_t r = next.fetch_add(1);
      if (r >= rows.size()) break;
      int y = rows[r];
      for (int x = 0; x < W; x++) {
        uint32_t pix = (uint32_t)y * (uint32_t)W + (uint32_t)x;
        float* a = accum + 3 * ((size_t)r * (size_t)W + (size_t)x);
        vec3 acc{a[0], a[1], a[2]};
        uint64_t rays0 = cnt.rays;
        for (int f = frame_begin; f < frame_begin + n_frames; f++) {
          int s_i = f % sq;
          int s_j = f / sq % sq;
          Rng g(seed, pix, (uint32_t)f, kTagPath);
          Ctx c{s, &g, &cnt};
          Ray ray = cam.GetRay(x, y, s_i, s_j, g);
          vec3 col = forward ? RayColorForward(c, ray, max_depth) : RayColor(c, ray, max_depth);
          acc = acc + col;
          draws[(size_t)tid] += g.draws;
        }
        a[0] = acc.x;
        a[1] = acc.y;
        a[2] = acc.z;
        if (ray_counts) ray_counts[(size_t)r * (size_t)W + (size_t)x] += (uint32_t)(cnt.rays - rays0);
      }
    }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < threads; t++) pool.emplace_back(work, t);
  work(0);
  for (auto& t : pool) t.join();
  if (out_cnt) {
    Counters tot;
    uint64_t d = 0;
    for (size_t i = 0; i < cnts.size(); i++) {
      tot.add(cnts[i]);
      d += draws[i];
    }
    *out_cnt = {tot.rays, tot.bvh, tot.quad, tot.sphere, tot.xform, tot.medium, tot.list, d};
  }
  return 0;
}

}  // extern "C"
