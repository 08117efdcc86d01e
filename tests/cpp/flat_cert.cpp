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
// The lane model is tests/cpp/kernel_model.h; the scenes and the rays are drawn by tests/cpp/gen_scenes.h.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "gen_scenes.h"

using namespace gen_scenes;

namespace {
struct Tally {
  long rays = 0, hits = 0, cert = 0, uncert = 0, decided = 0, decided_uncert = 0, bad = 0, nonfinite = 0;
};

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

void Report(const char* what, const V3& o, const V3& d, const Result& a, const Result& b) {
  fprintf(stderr, "%s\n o = (%a %a %a) d = (%a %a %a)\n bvh: prim %08x t %a\n flat: prim %08x t %a uncert %d xform %d\n", what,
          o.x, o.y, o.z, d.x, d.y, d.z, a.prim, a.t, b.prim, b.t, (int)b.uncert, (int)b.xform);
}

// Both walks of one ray; returns false on a certified disagreement or an unmodelled step.
bool OneRay(const CompiledScene& c, V3 o, V3 d, Tally& t, Result* bvh_out = nullptr) {
  if (!Finite3(o) || !Finite3(d)) return true;
  Result a, b;
  if (!Walk(c, {kLinWide, kEager, kFlatOn}, o, d, a) || !Walk(c, {kFlatWide, kEager, c.flat_mode}, o, d, b)) {
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
  return gen_scenes::RunRays(c, nray, [&](V3 o, V3 d, Result* hit) { return OneRay(c, o, d, t, hit); });
}

void Print(const std::string& name, const CompiledScene& c, const Tally& t) {
  printf("%s flat=%d steps=%d rays=%ld hits=%ld certified=%ld uncertified=%ld nonfinite=%ld decided=%ld decided_uncertified=%ld bad=%ld\n",
         name.c_str(), c.flat_wide.empty() ? 0 : 1, c.flat_steps, t.rays, t.hits, t.cert, t.uncert, t.nonfinite, t.decided,
         t.decided_uncert, t.bad);
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
    int leaves;
    const std::string path = dir + "/flat_cert_gen.json";
    if (!WriteFile(path, GeneratedScene(g, leaves))) return 2;
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
    if (!FourLeafRays([&](V3 o, V3 d) { return OneRay(c, o, d, t); })) return 1;
    Print("four_leaf", c, t);
  }
  return rc;
}
