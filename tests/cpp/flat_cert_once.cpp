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
// Scenes and rays are drawn as tests/cpp/flat_cert.cpp draws them (tests/cpp/gen_scenes.h): the files on the
// command line; generated scenes of 2 to 8 BVH leaves; the four-leaf scene with its rays. The walk with both
// evaluations is tests/cpp/kernel_model.h Walk, the one flat_cert.cpp walks.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "gen_scenes.h"

using namespace gen_scenes;

namespace {
struct Tally {
  long rays = 0, hits = 0, rule_uncert_xform = 0, rule_uncert_world = 0, nonfinite = 0, table_rows = 0, bad = 0;
};

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

// Both evaluations on one ray; returns false on a disagreement or an unmodelled step.
bool OneRay(const CompiledScene& c, V3 o, V3 d, Tally& t, Result* out = nullptr) {
  if (!Finite3(o) || !Finite3(d)) return true;
  Result a, b;
  if (!Walk(c, {kFlatWide, kEager, c.flat_mode}, o, d, a) || !Walk(c, {kFlatWide, kLazy, c.flat_mode}, o, d, b)) {
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

bool RunRays(const CompiledScene& c, long nray, Tally& t) {
  return gen_scenes::RunRays(c, nray, [&](V3 o, V3 d, Result* hit) { return OneRay(c, o, d, t, hit); });
}

void Print(const std::string& name, int flat, int steps, const Tally& t) {
  printf("%s flat=%d steps=%d rays=%ld hits=%ld rule_uncert_xform=%ld rule_uncert_world=%ld nonfinite=%ld table_rows=%ld bad=%ld\n",
         name.c_str(), flat, steps, t.rays, t.hits, t.rule_uncert_xform, t.rule_uncert_world, t.nonfinite, t.table_rows, t.bad);
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
    int leaves;
    const std::string path = dir + "/flat_cert_once_gen.json";
    if (!WriteFile(path, GeneratedScene(g, leaves))) return 2;
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
    if (!FourLeafRays([&](V3 o, V3 d) { return OneRay(c, o, d, t); })) return 1;
    Print("four_leaf", 1, c.flat_steps, t);
  }
  return 0;
}
