// Scenes and rays of the flat walk's host harnesses, once (flat_cert.cpp, flat_cert_once.cpp,
// flat_program_shape.cpp): one generator state, so a harness's output is a function of its seed and of the order
// in which its main draws scenes and rays. No draw may be added, dropped or reordered here.
// Scenes: generated scenes of 2 to 8 BVH leaves (walls with shared edges and corners, MakeBox boxes plain and
// rotated about y in different subtrees, thin boxes, integer coordinates, far-off coordinates where a quad's box
// padding is about 1 ulp of its plane); and the four-leaf scene in which the slab test decides every ray (a
// transformed box's model-space t culls the other subtree: Transform.cpp:13-20).
// Rays: through the scene's interior; aimed at edges and corners of the BVH nodes' boxes, on them and a few ulps
// beside; leaving a rounded hit point like a diffuse bounce (direction lengths 0.01 to 2); with zero, tiny and
// non-finite-reciprocal direction components; along box planes.
#pragma once
#include <cmath>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "kernel_model.h"

namespace gen_scenes {
using namespace kernel_model;

inline std::mt19937_64 rng;
inline float U(float lo, float hi) { return lo + (hi - lo) * (float)((rng() >> 11) * (1.0 / 9007199254740992.0)); }
inline V3 Dir(float len) {  // a direction of the given length
  V3 v;
  float l;
  do {
    v = V3{U(-1, 1), U(-1, 1), U(-1, 1)};
    l = Dot(v, v);
  } while (l > 1.0f || l < 1e-6f);
  const float s = len / std::sqrt(l);
  return V3{v.x * s, v.y * s, v.z * s};
}
inline float Len() { return std::exp(U(std::log(0.01f), std::log(2.0f))); }  // 0.01 .. 2, what the diffuse scatter produces

// The product's loader and compiler on a scene file.
inline bool Compile(const std::string& path, CompiledScene& c) {
  Scene s;
  std::string err;
  if (!LoadScene(path, 1, s, err) || !CompileScene(s, c, err)) {
    fprintf(stderr, "%s: %s\n", path.c_str(), err.c_str());
    return false;
  }
  return true;
}

inline bool WriteFile(const std::string& path, const std::string& text) {
  FILE* f = fopen(path.c_str(), "w");
  if (!f) return false;
  fputs(text.c_str(), f);
  fclose(f);
  return true;
}
inline std::string Vec(float x, float y, float z) {
  char b[128];
  snprintf(b, sizeof b, "[%.9g, %.9g, %.9g]", x, y, z);
  return b;
}
inline const char* const kHead = "{\"camera\": {\"center\": [0, 0, -10], \"look_at\": [0, 0, 0]}, \"materials\": [{\"type\": "
                                 "\"lambertian\", \"albedo\": [0.5, 0.5, 0.5]}], \"primitives\": [";

// The four-leaf scene: a unit-scale box rotated +10 degrees about y at the origin, two 30 x 30 quads
// at x = 200 and x = 400, the same box rotated -10 degrees at (600, 0, 0).
inline std::string FourLeafScene() {
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
// The four-leaf scene's rays: x = 1000, direction (-s, ~0, ~0), s in {0.1, 0.01}. one_ray(o, d) -> bool.
template <class OneRay>
bool FourLeafRays(OneRay one_ray) {
  for (int k = 0; k < 160000; k++) {
    const float s = (k & 1) ? 0.1f : 0.01f;
    const V3 o{1000.0f, U(5.0f, 160.0f), U(40.0f, 120.0f)};
    const V3 d{-s, U(-1e-4f, 1e-4f) * s, U(-1e-4f, 1e-4f) * s};
    if (!one_ray(o, d)) return false;
  }
  return true;
}

// A generated scene of `leaves` BVH leaves around `origin` at scale `sc`: walls on a shared grid of plane
// coordinates (shared edges and corners), plain boxes, thin boxes, boxes rotated about y.
inline std::string GeneratedScene(int leaves, float sc, const float origin[3], bool integer) {
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
// The g-th generated scene of a harness's run: 2 + g % 7 leaves, and by (g / 7) % 4 unit scale, scale 185, scale
// 555 with integer coordinates, or unit scale far from the origin.
inline std::string GeneratedScene(int g, int& leaves) {
  leaves = 2 + g % 7;
  const int cls = (g / 7) % 4;
  const float sc = cls == 0 ? 1.0f : cls == 1 ? 185.0f : cls == 2 ? 555.0f : 1.0f;
  const float far = cls == 3 ? 16384.0f : (cls == 2 ? 0.0f : U(-4.0f, 4.0f) * sc);
  const float origin[3] = {far, cls == 3 ? 4096.0f : 0.0f, -far};
  return GeneratedScene(leaves, sc, origin, cls == 2);
}

struct Box6 {
  float lo[3], hi[3];
};
inline std::vector<Box6> NodeBoxes(const CompiledScene& c) {
  std::vector<Box6> out;
  for (size_t i = 0; i < c.lin.size() / 4; i++) {
    if (c.lin[4 * i] != kBvh) continue;
    const float* r = &c.lind[4 * (size_t)c.lin[4 * i + 2]];
    out.push_back(Box6{{r[0], r[1], r[2]}, {r[4], r[5], r[6]}});
  }
  return out;
}

// nray rays of the six classes above against the scene's BVH node boxes, each given to the harness's check:
// one_ray(o, d, Result* hit) -> bool, false ends the run; `hit`, where not null, receives the ray's closest hit.
template <class OneRay>
bool RunRays(const CompiledScene& c, long nray, OneRay one_ray) {
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
      if (!one_ray(o, d, &h)) return false;
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
    if (!one_ray(o, d, (Result*)nullptr)) return false;
  }
  return true;
}
}  // namespace gen_scenes
