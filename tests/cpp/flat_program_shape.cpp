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
// gen_scenes.h: walls with shared edges and corners, MakeBox boxes plain and rotated about y, thin boxes,
// integer coordinates, far-off coordinates).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "gen_scenes.h"

using namespace gen_scenes;

namespace {
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
    int leaves;
    const std::string path = dir + "/flat_program_shape_gen.json";
    if (!WriteFile(path, GeneratedScene(g, leaves))) return 2;
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
