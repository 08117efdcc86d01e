// Digests of everything CompileScene produces, for every committed scene under every compile setting,
// host only:
//   compile_digest env|options <scene.json>...
// One line per scene and setting: "<file> <row> ok=<0|1>", then every scalar field of CompiledScene by
// value, a 64-bit FNV-1a digest of every vector (its length and its bytes) and one digest over all of
// them ("combined"). The rows: the defaults, lists not accelerated, each knob alone at its non-default
// value, balanced list trees (acc_depth_slack = 0) and the step limit at 10 and at the scene's own step
// count. Mode `env` sets the RT2_* variables and calls CompileScene; mode `options` fills a
// CompileOptions and calls CompileSceneWith: both must print the same lines. tests/test_compile_digest.py
// compares them with tests/golden/compiled_scene_digests.json, recorded from the commit before the
// compiler was split into passes by this program built with -DDIGEST_PARENT (env mode only, the old
// CompileSceneWith(bool, int) for the slack row, and no step-limit rows: that commit read the limit once
// per process and overflowed the heap below it).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "scene.h"

using namespace rt2;

namespace {

struct Fnv {
  uint64_t h = 0xcbf29ce484222325ull;
  void Bytes(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
  }
  void U64(uint64_t v) { Bytes(&v, 8); }
};

struct Row {
  const char* name;
  const char* var;  // environment variable of the knob, or nullptr
  const char* value;
};
const Row kKnobs[] = {{"flat_bvh=0", "RT2_FLAT_BVH", "0"},       {"flat_bvh=2", "RT2_FLAT_BVH", "2"},
                      {"box_aa=0", "RT2_BOX_AA", "0"},           {"bvh_pairs=0", "RT2_BVH_PAIRS", "0"},
                      {"acc_octants=0", "RT2_ACC_OCTANTS", "0"}, {"acc_sah=0", "RT2_ACC_SAH", "0"},
                      {"hit_table=0", "RT2_HIT_TABLE", "0"}};
const char* const kVars[] = {"RT2_FLAT_BVH",    "RT2_BOX_AA",    "RT2_BVH_PAIRS",       "RT2_ACC_OCTANTS",
                             "RT2_ACC_SAH",     "RT2_HIT_TABLE", "RT2_LINEAR_MAX_STEPS"};

template <class T>
void Vec(const char* name, const std::vector<T>& v, Fnv& all) {
  Fnv f;
  f.U64(v.size());
  f.Bytes(v.data(), v.size() * sizeof(T));
  all.U64(f.h);
  std::printf(" %s=%016llx", name, (unsigned long long)f.h);
}
void Scalar(const char* name, long long v, Fnv& all) {
  all.U64((uint64_t)v);
  std::printf(" %s=%lld", name, v);
}

void Print(const char* path, const char* row, bool ok, const CompiledScene& c) {
  const char* base = std::strrchr(path, '/');
  std::printf("%s %s ok=%d steps=%zu", base ? base + 1 : path, row, ok ? 1 : 0, c.lin.size() / 4);
  Fnv all;
  Scalar("hot_records", c.hot_records, all);
  Scalar("root", c.root, all);
  Scalar("max_stack", c.max_stack, all);
  Scalar("stack_ok", c.stack_ok, all);
  Scalar("lin_xform_depth", c.lin_xform_depth, all);
  Scalar("bvh_nodes", c.bvh_nodes, all);
  Scalar("quads", c.quads, all);
  Scalar("spheres", c.spheres, all);
  Scalar("lists", c.lists, all);
  Scalar("xforms", c.xforms, all);
  Scalar("media", c.media, all);
  Scalar("acc_lists", c.acc_lists, all);
  Scalar("acc_nodes", c.acc_nodes, all);
  Scalar("box_steps", c.box_steps, all);
  Scalar("bvh_depth", c.bvh_depth, all);
  Scalar("features", c.features, all);
  Scalar("origins_bounded", c.origins_bounded, all);
  Scalar("flat_mode", c.flat_mode, all);
  Scalar("flat_steps", c.flat_steps, all);
  Vec("nodes", c.nodes, all);
  Vec("materials", c.materials, all);
  Vec("textures", c.textures, all);
  Vec("perlin_vec", c.perlin_vec, all);
  Vec("perlin_perm", c.perlin_perm, all);
  Vec("lin", c.lin, all);
  Vec("lind", c.lind, all);
  Vec("lin_wide", c.lin_wide, all);
  Vec("hit", c.hit, all);
  Vec("flat_wide", c.flat_wide, all);
  Vec("flat_cert", c.flat_cert, all);
  std::printf(" combined=%016llx\n", (unsigned long long)all.h);
}

void ClearEnv() {
  for (const char* v : kVars) unsetenv(v);
}

#ifndef DIGEST_PARENT
// the option field a knob's variable sets, as CompileOptions::FromEnv reads it
void SetOption(CompileOptions& o, const char* var, const char* value) {
  const int v = std::atoi(value);
  const std::string n = var;
  if (n == "RT2_FLAT_BVH") o.flat_bvh = v;
  if (n == "RT2_BOX_AA") o.box_aa = v != 0;
  if (n == "RT2_BVH_PAIRS") o.bvh_pairs = v != 0;
  if (n == "RT2_ACC_OCTANTS") o.acc_octants = v != 0;
  if (n == "RT2_ACC_SAH") o.acc_sah = v != 0;
  if (n == "RT2_HIT_TABLE") o.hit_table = v != 0;
}
#endif

int Digest(const char* path, bool env) {
  Scene s;
  std::string err;
  if (!LoadScene(path, 0x5EED2024ull, s, err)) {
    std::fprintf(stderr, "load %s: %s\n", path, err.c_str());
    return 2;
  }
  ClearEnv();
  CompiledScene c;
  bool ok = CompileScene(s, c, err);
  Print(path, "default", ok, c);
  const size_t steps = c.lin.size() / 4;
  (void)steps;
#ifdef DIGEST_PARENT
  (void)env;
  ok = CompileScene(s, c, err, false);
  Print(path, "lists_plain", ok, c);
  for (const Row& r : kKnobs) {
    setenv(r.var, r.value, 1);
    ok = CompileScene(s, c, err);
    Print(path, r.name, ok, c);
    ClearEnv();
  }
  ok = CompileSceneWith(s, c, err, true, 0);
  Print(path, "acc_depth_slack=0", ok, c);
#else
  // one row: the variable set (env) or the option changed (options), lists accelerated or not
  auto row = [&](const char* name, const char* var, const char* value, bool lists, int slack) {
    if (env) {
      if (var) setenv(var, value, 1);
      if (slack == kAccDepthSlack) {
        ok = CompileScene(s, c, err, lists);
      } else {  // (no variable sets the slack)
        CompileOptions o = CompileOptions::FromEnv();
        o.accelerate_lists = lists;
        o.acc_depth_slack = slack;
        ok = CompileSceneWith(s, c, err, o);
      }
      ClearEnv();
    } else {
      CompileOptions o;
      o.accelerate_lists = lists;
      o.acc_depth_slack = slack;
      if (var && std::string(var) == "RT2_LINEAR_MAX_STEPS") o.linear_max_steps = std::strtoul(value, nullptr, 10);
      else if (var) SetOption(o, var, value);
      ok = CompileSceneWith(s, c, err, o);
    }
    Print(path, name, ok, c);
  };
  row("lists_plain", nullptr, nullptr, false, kAccDepthSlack);
  for (const Row& r : kKnobs) row(r.name, r.var, r.value, true, kAccDepthSlack);
  row("acc_depth_slack=0", nullptr, nullptr, true, 0);
  row("linear_max_steps=10", "RT2_LINEAR_MAX_STEPS", "10", true, kAccDepthSlack);
  row("linear_max_steps=own", "RT2_LINEAR_MAX_STEPS", std::to_string(steps).c_str(), true, kAccDepthSlack);
#endif
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (argc < 3 || (mode != "env" && mode != "options")) {
    std::fprintf(stderr, "usage: compile_digest env|options <scene.json>...\n");
    return 2;
  }
#ifdef DIGEST_PARENT
  if (mode != "env") return 2;
#endif
  for (int a = 2; a < argc; a++) {
    const int rc = Digest(argv[a], mode == "env");
    if (rc != 0) return rc;
  }
  return 0;
}
