// The hit table of the threaded program (rt2_layout.h HIT, compile.cpp BuildHitTable) against the words
// the global-memory path reads, host only:
//   hit_table <scene.json>...
// For every scene: each quad step's hit record must equal, bit for bit, what render.hip's chain reads
// for that primitive: the transform's ref from the trace's tail, the normal(s) and the material index of
// resolve_hit from `lind`, the material's two records of `materials`, and, for a material that reads a
// solid texture, tex_value's record of `textures`; each XFORM step's entry must equal its lind record.
// The table is addressed by the primitive's own record offset, so every quad step's offset must lie
// in the table with its kHitRecords records, no two entries may overlap, and every other word is 0. A
// scene without a table must have a reason (no program, nested transforms, no quad, too large), and
// RT2_HIT_TABLE=0 in the environment must build none. Prints one line per scene,
// "<file> hit_bytes=<n> quads=<n> xforms=<n> depth=<n>", and exits non-zero on the first violation.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "scene.h"

using namespace rt2;

static uint32_t U(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

static int fail(const char* scene, const char* what, size_t i) {
  std::fprintf(stderr, "%s: violation at step %zu: %s\n", scene, i, what);
  return 1;
}

static int check(const char* path) {
  Scene s;
  std::string err;
  if (!LoadScene(path, 0x5EED2024ull, s, err)) {
    std::fprintf(stderr, "load %s: %s\n", path, err.c_str());
    return 2;
  }
  unsetenv("RT2_HIT_TABLE");
  CompiledScene c;
  if (!CompileScene(s, c, err)) {
    std::fprintf(stderr, "compile %s: %s\n", path, err.c_str());
    return 2;
  }
  const size_t n = c.lin.size() / 4;
  size_t quads = 0, xforms = 0;
  for (size_t i = 0; i < n; i++) {
    quads += c.lin[4 * i] == kQuad;
    xforms += c.lin[4 * i] == kXform;
  }
  if (c.hit.empty()) {
    const bool reason = n == 0 || quads == 0 || c.lin_xform_depth > 1 || c.lind.size() * 4 > kHitTableBytesMax;
    if (!reason) return fail(path, "no table and no reason for it", 0);
  } else {
    if (c.hit.size() != c.lind.size()) return fail(path, "the table is not as long as lind", 0);
    if (c.hit.size() * 4 > kHitTableBytesMax || c.lin_xform_depth > 1) return fail(path, "a table that must not be built", 0);
    std::vector<char> used(c.hit.size(), 0);
    auto claim = [&](size_t w0, size_t words) {
      if (w0 + words > c.hit.size()) return false;
      for (size_t k = 0; k < words; k++) {
        if (used[w0 + k]) return false;
        used[w0 + k] = 1;
      }
      return true;
    };
    for (size_t i = 0; i < n; i++) {
      const uint32_t kind = c.lin[4 * i];
      const size_t off = 4 * (size_t)c.lin[4 * i + 2];
      if (kind == kXform) {
        if (!claim(off, 4 * kXformRecords)) return fail(path, "transform entry outside the table or overlapping", i);
        if (std::memcmp(&c.hit[off], &c.lind[off], 16 * kXformRecords) != 0) return fail(path, "transform entry", i);
        continue;
      }
      if (kind != kQuad) continue;
      if (!claim(off, 4 * kHitRecords)) return fail(path, "hit record outside the table or overlapping", i);
      const float* N = c.lind.data();
      const float* h = &c.hit[off];
      const uint32_t code = c.lin[4 * i + 1] & 7u;  // the step's axis code: 4..6 = QUADAA layout
      uint32_t want[4 * kHitRecords] = {0};
      uint32_t mat, xf;
      if (code >= 4 && code <= 6) {
        xf = U(N[off + 4 * 4 + 1]);                                    // trace tail: word(off + 4, 1)
        for (int k = 0; k < 3; k++) want[k] = U(N[off + 4 * 2 + k]);   // resolve_hit: N[off + 2].xyz
        mat = U(N[off + 4 * 3 + 3]);                                   // N[off + 3].w
        if (xf != kRefNone) {
          for (int k = 0; k < 3; k++) want[4 + k] = U(N[off + 4 * 3 + k]);  // the world normal, N[off + 3].xyz
          want[7] |= kHitWorldNormal;
        }
      } else {
        xf = U(N[off + 4 * 3 + 3]);                                    // word(off + 3, 3)
        for (int k = 0; k < 3; k++) want[k] = U(N[off + k]);           // N[off].xyz
        mat = U(N[off + 4 * 1 + 3]);                                   // word(off + 1, 3)
      }
      want[3] = xf;
      if (xf != kRefNone) {
        // the ref is a transform of this program whose entry is in the table
        bool found = false;
        for (size_t j = 0; j < n; j++)
          found = found || (c.lin[4 * j] == kXform && make_ref(kXform, c.lin[4 * j + 2]) == xf);
        if (!found) return fail(path, "the record's transform is no XFORM step", i);
      }
      if (8 * (size_t)mat + 8 > c.materials.size()) return fail(path, "material index", i);
      for (int k = 0; k < 8; k++) want[8 + k] = U(c.materials[8 * (size_t)mat + k]);  // materials[2 mat], [2 mat + 1]
      const uint32_t type = want[8], tex = want[14];
      if ((type == kMatTexture || type == kMatDiffuseLight || type == kMatIsotropic) &&
          12 * (size_t)tex + 12 <= c.textures.size() && U(c.textures[12 * (size_t)tex]) == kTexSolid) {
        for (int k = 0; k < 4; k++) want[16 + k] = U(c.textures[12 * (size_t)tex + k]);  // tex_value: T[3 idx]
        want[7] |= kHitSolid;
      }
      for (int k = 0; k < 4 * kHitRecords; k++)
        if (U(h[k]) != want[k]) {
          std::fprintf(stderr, "word %d: %08x, the chain reads %08x\n", k, U(h[k]), want[k]);
          return fail(path, "hit record", i);
        }
    }
    for (size_t w = 0; w < c.hit.size(); w++)
      if (!used[w] && U(c.hit[w]) != 0u) return fail(path, "a word outside every entry is not 0", w);
  }
  std::printf("%s hit_bytes=%zu quads=%zu xforms=%zu depth=%d\n", path, c.hit.size() * 4, quads, xforms, c.lin_xform_depth);
  // the switch, through the environment and as an option
  setenv("RT2_HIT_TABLE", "0", 1);
  CompiledScene off, off2;
  if (!CompileScene(s, off, err)) return 2;
  unsetenv("RT2_HIT_TABLE");
  if (!off.hit.empty()) return fail(path, "RT2_HIT_TABLE=0 built a table", 0);
  CompileOptions no_table;
  no_table.hit_table = false;
  if (!CompileSceneWith(s, off2, err, no_table)) return 2;
  if (!off2.hit.empty() || off2.lin != off.lin) return fail(path, "hit_table = false differs from RT2_HIT_TABLE=0", 0);
  // (bytes, not floats: refs such as kRefNone are NaN patterns)
  if (off.lind.size() != c.lind.size() || std::memcmp(off.lind.data(), c.lind.data(), 4 * c.lind.size()) != 0 ||
      off.lin != c.lin)
    return fail(path, "RT2_HIT_TABLE=0 changed the program", 0);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  for (int a = 1; a < argc; a++) {
    const int rc = check(argv[a]);
    if (rc != 0) return rc;
  }
  return 0;
}
