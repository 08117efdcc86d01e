// query_host.cpp — the ray queries' host side (raytrace2_amd/csrc/query.h, launch_plan.h PlanQuery) without a
// GPU: QueryRayValid on every word's NaN, infinities and zeros, on d = 0, on the ends of the interval, of the time
// and of every declared domain bound with the next float beyond each; PlanQuery over n at the wave edges and at
// 2^31 - 1, with and without a threaded program, for every feature set the kernels are instantiated for. A
// stand-alone program: tests/test_query_host.py builds it plain and with the host sanitizers. Exit status 0: all
// passed.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <limits>

#include "launch_plan.h"
#include "query.h"

using namespace rt2;

static int g_failed = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      if (g_failed++ < 20) {                     \
        fprintf(stderr, "FAILED %s: ", #cond);   \
        fprintf(stderr, __VA_ARGS__);            \
        fprintf(stderr, "\n");                   \
      }                                          \
    }                                            \
  } while (0)

struct Ray {
  float w[8];
};
static Ray Good() { return Ray{{1.0f, 2.0f, 3.0f, FLT_MAX, 0.0f, 0.6f, -0.8f, 0.5f}}; }
static float Up(float x) { return std::nextafter(x, INFINITY); }
static float Down(float x) { return std::nextafter(x, -INFINITY); }

static void CheckValid() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = INFINITY;
  CHECK(QueryRayValid(Good().w), "the good ray");
  for (int k = 0; k < 8; k++) {
    for (float bad : {nan, inf, -inf}) {
      Ray r = Good();
      r.w[k] = bad;
      CHECK(!QueryRayValid(r.w), "word %d = %f", k, (double)bad);
    }
    for (float z : {0.0f, -0.0f}) {
      Ray r = Good();
      r.w[k] = z;
      // a zero is fine everywhere but in tmax (0.001 < tmax); the direction keeps its other components
      CHECK(QueryRayValid(r.w) == (k != kQrTmax), "word %d = %s0", k, std::signbit(z) ? "-" : "+");
    }
  }
  {  // d = 0, in every combination of signs
    for (int s = 0; s < 8; s++) {
      Ray r = Good();
      for (int k = 0; k < 3; k++) r.w[kQrDx + k] = (s >> k) & 1 ? -0.0f : 0.0f;
      CHECK(!QueryRayValid(r.w), "d = 0 (signs %d)", s);
    }
  }
  {  // tmax: (0.001, FLT_MAX]
    Ray r = Good();
    r.w[kQrTmax] = 0.001f;
    CHECK(!QueryRayValid(r.w), "tmax = 0.001");
    r.w[kQrTmax] = Up(0.001f);
    CHECK(QueryRayValid(r.w), "tmax just above 0.001");
    r.w[kQrTmax] = FLT_MAX;
    CHECK(QueryRayValid(r.w), "tmax = FLT_MAX");
    r.w[kQrTmax] = -1.0f;
    CHECK(!QueryRayValid(r.w), "tmax < 0");
  }
  {  // time: [0, 1]
    Ray r = Good();
    for (float t : {-0.0f, 0.0f, 1.0f}) {
      r.w[kQrTime] = t;
      CHECK(QueryRayValid(r.w), "time %f", (double)t);
    }
    r.w[kQrTime] = Up(1.0f);
    CHECK(!QueryRayValid(r.w), "time just above 1");
    r.w[kQrTime] = Down(-0.0f);  // the first float below zero
    CHECK(!QueryRayValid(r.w), "time just below 0");
  }
  // the origin bound, both ends and the next float beyond, on every axis
  CHECK(kQueryOriginMax == 0x1p64f, "origin bound");
  for (int k = 0; k < 3; k++) {
    for (float s : {1.0f, -1.0f}) {
      Ray r = Good();
      r.w[kQrOx + k] = s * kQueryOriginMax;
      CHECK(QueryRayValid(r.w), "origin %d at %c2^64", k, s > 0 ? '+' : '-');
      r.w[kQrOx + k] = s * Up(kQueryOriginMax);
      CHECK(!QueryRayValid(r.w), "origin %d beyond %c2^64", k, s > 0 ? '+' : '-');
    }
  }
  // the direction bounds: on the largest component, whichever axis holds it and whatever its sign
  CHECK(kQueryDirMaxLow == 0x1p-20f && kQueryDirMaxHigh == 0x1p20f, "direction bounds");
  for (int k = 0; k < 3; k++) {
    for (float s : {1.0f, -1.0f}) {
      Ray r = Good();
      for (int j = 0; j < 3; j++) r.w[kQrDx + j] = 0.0f;
      r.w[kQrDx + k] = s * kQueryDirMaxHigh;
      r.w[kQrDx + (k + 1) % 3] = -s * 0.5f;
      CHECK(QueryRayValid(r.w), "largest component %d at 2^20", k);
      r.w[kQrDx + k] = s * Up(kQueryDirMaxHigh);
      CHECK(!QueryRayValid(r.w), "largest component %d beyond 2^20", k);
      r.w[kQrDx + (k + 1) % 3] = s * 0x1p-30f;  // a smaller component below the low bound is fine
      r.w[kQrDx + k] = s * kQueryDirMaxLow;
      CHECK(QueryRayValid(r.w), "largest component %d at 2^-20", k);
      r.w[kQrDx + k] = s * Down(kQueryDirMaxLow);
      CHECK(!QueryRayValid(r.w), "largest component %d below 2^-20", k);
    }
  }
  // the domain holds unit directions along every axis and diagonal, and directions of a camera's scale
  for (float x : {-1.0f, 0.0f, 1.0f})
    for (float y : {-1.0f, 0.0f, 1.0f})
      for (float z : {-1.0f, 0.0f, 1.0f}) {
        if (x == 0.0f && y == 0.0f && z == 0.0f) continue;
        const float l = std::sqrt(x * x + y * y + z * z);
        Ray r = Good();
        r.w[kQrDx] = x / l, r.w[kQrDy] = y / l, r.w[kQrDz] = z / l;
        CHECK(QueryRayValid(r.w), "unit direction %g %g %g", (double)x, (double)y, (double)z);
        r.w[kQrDx] = x * 800.0f, r.w[kQrDy] = y * 800.0f, r.w[kQrDz] = z * 800.0f;
        CHECK(QueryRayValid(r.w), "camera-scale direction");
      }
}

static void CheckPlan() {
  // the feature sets of render.hip kVariants, in its order
  const uint32_t kBook2 = kFeatSphere | kFeatMedium | kFeatXform | kFeatNoise | kFeatSpecular | kFeatAccList | kFeatMotion;
  const uint32_t variants[] = {kFeatXform, kFeatXform | kFeatMedium, kFeatSphere | kFeatSpecular | kFeatDefocus, kBook2,
                               kFeatAll};
  const size_t kCuLds = 160 * 1024, kGroupLds = 64 * 1024;
  const int block = 256;
  for (uint32_t n : {1u, 63u, 64u, 65u, 0x7FFFFFFFu}) {
    for (int v = 0; v < 5; v++) {
      for (uint32_t lin_len : {0u, 29u}) {
        for (int depth : {1, kTraversalStack, kTraversalStack + 1}) {
          const QueryPlan q = PlanQuery(lin_len, v, variants[v], depth, n, block);
          CHECK(q.threaded == (lin_len != 0), "traversal");
          CHECK(q.variant == (q.threaded ? v : -1), "variant %d", q.variant);
          CHECK(q.ok == (q.threaded || depth <= kTraversalStack), "ok at depth %d", depth);
          // the grid covers n, in whole waves, with less than one workgroup to spare
          const uint64_t lanes = (uint64_t)q.grid * (uint64_t)block;
          CHECK(lanes >= n && lanes - n < (uint64_t)block + 64, "grid %u for n %u", q.grid, n);
          CHECK(lanes <= 0x80000000ull, "lane index overflows 32 bits: %llu", (unsigned long long)lanes);
          // the records' float4 indices (2 per ray in, 4 per ray out) are 64-bit in the kernel; the byte sizes fit
          CHECK((uint64_t)n * kQueryHitFloats * 4 < (1ull << 40), "bytes");
          if (q.ok) {
            CHECK(q.lds_dynamic + q.lds_static <= kGroupLds && q.lds_dynamic + q.lds_static <= kCuLds, "LDS %zu + %zu",
                  q.lds_dynamic, q.lds_static);
          }
          CHECK(q.lds_dynamic == (q.threaded ? 0u : (size_t)depth * block * 4), "dynamic LDS");
          const bool planes = q.threaded && (variants[v] & kFeatMedium) && !(variants[v] & kFeatSphere);
          CHECK(q.lds_static == (planes ? (size_t)(block / 64) * kBoundaryAAMax * 64 * 4 : 0u), "static LDS");
        }
      }
    }
  }
  CHECK(QueryGrid(1, 256) == 1 && QueryGrid(256, 256) == 1 && QueryGrid(257, 256) == 2, "grid edges");
  CHECK(QueryGrid(0x7FFFFFFFu, 256) == 0x800000u, "grid at 2^31 - 1");
}

int main() {
  CheckValid();
  CheckPlan();
  if (g_failed) {
    fprintf(stderr, "%d checks failed\n", g_failed);
    return 1;
  }
  printf("query host ok\n");
  return 0;
}
