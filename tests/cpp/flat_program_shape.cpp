// Host check of the premise of the flat walk's scalar step index (render.hip trace_linear with kFlat,
// rt2_layout.h "Flat program", DESIGN.md §4 "The step index as a scalar"): in every flat program the compiler
// emits, no step sends lanes to different places, so the wave's step is a value of the step words alone.
//   flat_program_shape <scratch_dir> <seed> <generated_scenes> [scene.json ...]
// Every scene is loaded and compiled by the product (scene.cpp, compile.cpp). For a scene that got a flat
// program, on flat_wide:
//   * every entry's kind is kQuad, kXform, kXformExit or kProgramEnd (no kBvh skip, no sphere, medium or
//     accelerated list: the kinds that set a per-lane next), and kProgramEnd is the entry at flat_steps only;
//   * a kQuad entry's successor at + (aux & kRunLenMask) and every other entry's successor at + 1 land on an
//     entry start: past the entry, at most flat_steps (the kProgramEnd entry), and a run's entries are quads;
//   * following the successors from 0 reaches kProgramEnd in at most flat_steps moves, visiting each
//     transform's entry and its exit exactly once, entry before exit, no transform inside another.
// One line per scene: flat, steps, moves of the walk, transforms. Any violation is printed and the exit status
// is 1.
// Scenes: the files on the command line, and generated scenes of 2 to 8 BVH leaves (the generator of
// flat_cert.cpp: walls with shared edges and corners, MakeBox boxes plain and rotated about y, thin boxes,
// integer coordinates, far-off coordinates).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "scene.h"

using namespace rt2;

namespace {
std::mt19937_64 rng;
float U(float lo, float hi) { return lo + (hi - lo) * (float)((rng() >> 11) * (1.0 / 9007199254740992.0)); }

bool Compile(const std::string& path, CompiledScene& c) {
  Scene s;
  std::string err;
  if (!LoadScene(path, 1, s, err) || !CompileScene(s, c, err)) {
    fprintf(stderr, "%s: %s\n", path.c_str(), err.c_str());
    return false;
  }
  return true;
}

struct Shape {
  int moves = 0, xforms = 0, quad_steps = 0;
};

// The three properties above; `what` names the scene in a violation's message.
bool CheckShape(const CompiledScene& c, const std::string& what, Shape& out) {
  auto fail = [&](size_t at, const char* msg) {
    fprintf(stderr, "%s: entry %zu: %s\n", what.c_str(), at, msg);
    return false;
  };
  if (c.flat_steps <= 0 || c.flat_wide.size() != 16 * ((size_t)c.flat_steps + 1)) return fail(0, "flat_wide is not flat_steps + 1 entries");
  const size_t m = (size_t)c.flat_steps;
  auto kind = [&](size_t j) { return c.flat_wide[16 * j]; };
  auto succ = [&](size_t j) { return kind(j) == kQuad ? j + (c.flat_wide[16 * j + 3] & kRunLenMask) : j + 1; };
  if (kind(m) != kProgramEnd) return fail(m, "the last entry is not kProgramEnd");
  int xform_entries = 0, xform_exits = 0;
  for (size_t j = 0; j < m; j++) {
    const uint32_t k = kind(j);
    if (k != kQuad && k != kXform && k != kXformExit) return fail(j, k == kProgramEnd ? "kProgramEnd before the end" : "a kind that sets a per-lane next");
    xform_entries += k == kXform;
    xform_exits += k == kXformExit;
    const size_t s = succ(j);
    if (s <= j || s > m) return fail(j, "the successor is not an entry start of the program");
    if (k == kQuad)
      for (size_t q = j + 1; q < s; q++)
        if (kind(q) != kQuad) return fail(j, "the run covers an entry that is no quad");
  }
  // the walk from 0
  size_t at = 0;
  int moves = 0, entered = 0, left = 0;
  uint32_t open = kRefNone;  // the record of the transform the walk is in
  while (kind(at) != kProgramEnd) {
    if (moves >= c.flat_steps) return fail(at, "kProgramEnd not reached in flat_steps moves");
    const uint32_t* w = &c.flat_wide[16 * at];
    if (w[0] == kXform) {
      if (open != kRefNone) return fail(at, "a transform entered inside another");
      open = w[2];
      entered++;
    } else if (w[0] == kXformExit) {
      if (open == kRefNone || open != w[2]) return fail(at, "an exit without its transform's entry");
      if (w[3] != kRefNone) return fail(at, "an exit into a parent transform");
      open = kRefNone;
      left++;
    } else {
      out.quad_steps++;
    }
    at = succ(at);
    moves++;
  }
  if (at != m) return fail(at, "the walk ends before the last entry");
  if (open != kRefNone) return fail(at, "a transform left open at the end");
  // every transform step of the program lies on the walk (the walk never revisits: its index only grows)
  if (entered != xform_entries || left != xform_exits || entered != left || entered != c.xforms)
    return fail(at, "the walk does not visit each transform's entry and exit exactly once");
  out.moves = moves;
  out.xforms = entered;
  return true;
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
  if (argc < 4) {
    fprintf(stderr, "usage: flat_program_shape <scratch_dir> <seed> <generated_scenes> [scene.json ...]\n");
    return 2;
  }
  const std::string dir = argv[1];
  rng.seed(strtoull(argv[2], nullptr, 10));
  const int ngen = atoi(argv[3]);
  unsetenv("RT2_FLAT_BVH");
  // the committed scenes on the command line
  for (int i = 4; i < argc; i++) {
    CompiledScene c;
    if (!Compile(argv[i], c)) return 2;
    std::string name = argv[i];
    name = name.substr(name.find_last_of('/') + 1);
    Shape s;
    if (!c.flat_wide.empty() && !CheckShape(c, name, s)) return 1;
    printf("scene:%s flat=%d steps=%d moves=%d xforms=%d quad_steps=%d\n", name.c_str(), c.flat_wide.empty() ? 0 : 1,
           c.flat_steps, s.moves, s.xforms, s.quad_steps);
  }
  // generated scenes
  int gen_flat = 0, gen_xforms = 0, gen_moves = 0, gen_steps = 0, leaves_seen = 0;
  for (int g = 0; g < ngen; g++) {
    const int leaves = 2 + g % 7;
    const int cls = (g / 7) % 4;
    const float sc = cls == 0 ? 1.0f : cls == 1 ? 185.0f : cls == 2 ? 555.0f : 1.0f;
    const float far = cls == 3 ? 16384.0f : (cls == 2 ? 0.0f : U(-4.0f, 4.0f) * sc);
    const float origin[3] = {far, cls == 3 ? 4096.0f : 0.0f, -far};
    const std::string path = dir + "/flat_program_shape_gen.json";
    if (!WriteFile(path, GeneratedScene(leaves, sc, origin, cls == 2))) return 2;
    CompiledScene c;
    if (!Compile(path, c)) return 2;
    if (c.flat_wide.empty()) continue;
    Shape s;
    if (!CheckShape(c, "generated scene " + std::to_string(g), s)) {
      fprintf(stderr, "generated scene %d (%d leaves) kept at %s\n", g, leaves, path.c_str());
      return 1;
    }
    gen_flat++;
    gen_xforms += s.xforms;
    gen_moves += s.moves;
    gen_steps += c.flat_steps;
    leaves_seen |= 1 << leaves;
  }
  printf("generated flat=%d steps=%d moves=%d xforms=%d leaves_mask=%d\n", gen_flat, gen_steps, gen_moves, gen_xforms, leaves_seen);
  return 0;
}
