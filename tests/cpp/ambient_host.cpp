// Host evaluation of raytrace2_amd/csrc/ambient.h and of launch_plan.h PlanAmbient (no GPU).
//   ambient_host                 self-checks: the guard, the plan's sample ranges at the edges of 2^31 work items
//   ambient_host rays IN OUT     IN: rows of 11 floats (a point record, a unit-vector draw); OUT: rows of 10 floats:
//                                the ray record AmbientRay builds, QueryRayValid of the point, QueryRayValid of the ray
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ambient.h"
#include "launch_plan.h"

using namespace rt2;

static int failures = 0;
#define EXPECT(c)                                                   \
  do {                                                              \
    if (!(c)) {                                                     \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);            \
      failures++;                                                   \
    }                                                               \
  } while (0)

static void CheckGuard() {
  const float n[3] = {0.0f, 1.0f, 0.0f};
  const float opposite[3] = {-0.0f, -1.0f, 0.0f};  // u = -n: v = 0, the guard takes n
  float d[3];
  AmbientDirection(n, opposite, d);
  EXPECT(d[0] == 0.0f && d[1] == 1.0f && d[2] == 0.0f);
  const float edge[3] = {1e-8f, 1e-8f, -1e-8f}, above[3] = {1e-8f, 1.0000001e-8f, 0.0f};
  EXPECT(AmbientNearZero(edge) && !AmbientNearZero(above));
  EXPECT(kAmbientFrame0 == 0x80000000u && kAmbientInvalid == 0xFFFFFFFFu);
  const AmbientSource f = AmbientFeatureSource(nullptr, 2.0f, 37u), r = AmbientRecordSource(nullptr, 128u);
  EXPECT(f.stride == 16u && f.off_p == 2u && f.off_n == 5u && f.width == 37u && f.radius == 2.0f);
  EXPECT(r.stride == 8u && r.off_p == 0u && r.off_n == 4u && r.width == 0u && r.index0 == 128u && f.index0 == 0u);
}

static void CheckPlan() {
  const uint32_t points[] = {1u, 63u, 64u, 576u, 1u << 20, (1u << 22) + 64u, 0x7FFFFFFFu / 65535u, 0x7FFFFFFFu / 65535u + 1u,
                             1u << 30, 0x7FFFFFFFu};
  const uint32_t samples[] = {1u, 24u, 63u, 64u, 65u, 130u, 4096u, 65535u};
  for (uint32_t n : points)
    for (uint32_t k : samples)
      for (uint32_t lin_len : {0u, 100u}) {
        const AmbientPlan a = PlanAmbient(lin_len, 1, kFeatXform | kFeatMedium, 8, n, k, 256);
        EXPECT(a.per_launch >= 1u && a.per_launch <= k && a.last >= 1u && a.last <= a.per_launch);
        EXPECT((uint64_t)n * a.per_launch <= 0x7FFFFFFFull);
        EXPECT((uint64_t)(a.launches - 1u) * a.per_launch + a.last == k);
        EXPECT(a.launches == 1u || (uint64_t)n * (a.per_launch + 1u) > 0x7FFFFFFFull);  // no shorter range than needed
        EXPECT(a.q.ok && a.q.threaded == (lin_len != 0u) && a.q.variant == (lin_len ? 1 : -1));
        EXPECT((uint64_t)a.q.grid * 256u >= (uint64_t)n * a.per_launch);
        const Magic m = MakeMagic(a.per_launch);
        for (uint64_t w : {(uint64_t)0, (uint64_t)a.per_launch - 1u, (uint64_t)a.per_launch, (uint64_t)n * a.per_launch - 1u})
          EXPECT((uint32_t)((w * m.m) >> m.s) == (uint32_t)(w / a.per_launch));
      }
  EXPECT(!PlanAmbient(0u, 4, kFeatAll, kTraversalStack + 1, 10u, 4u, 256).q.ok);
}

static int Rays(const char* in_path, const char* out_path) {
  std::FILE* in = std::fopen(in_path, "rb");
  if (!in) return 2;
  std::vector<float> rows;
  float row[11];
  while (std::fread(row, sizeof(float), 11, in) == 11) rows.insert(rows.end(), row, row + 11);
  std::fclose(in);
  std::FILE* out = std::fopen(out_path, "wb");
  if (!out) return 2;
  for (size_t k = 0; k + 11 <= rows.size(); k += 11) {
    float o[10];
    AmbientRay(&rows[k], &rows[k + 8], o);
    o[8] = QueryRayValid(&rows[k]) ? 1.0f : 0.0f;
    o[9] = QueryRayValid(o) ? 1.0f : 0.0f;
    if (std::fwrite(o, sizeof(float), 10, out) != 10) return 2;
  }
  return std::fclose(out) == 0 ? 0 : 2;
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "rays")) return Rays(argv[2], argv[3]);
  CheckGuard();
  CheckPlan();
  if (failures) return 1;
  std::printf("ambient host ok\n");
  return 0;
}
