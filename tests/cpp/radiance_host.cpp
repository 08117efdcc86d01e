// Host evaluation of raytrace2_amd/csrc/radiance.h and of launch_plan.h PlanRadiance (no GPU): the plan's ranges
// cover every (ray, sample) once within both bounds, under bounds that force sample splits, ray splits and both; the
// waves' blocks cover a launch's items once; the ordered sum over split sample ranges equals the one-pass sum bit for
// bit on values whose addition order matters; validity is QueryRayValid; the item map, the stream words and the
// argument checks.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "launch_plan.h"
#include "radiance.h"

using namespace rt2;

static int failures = 0;
#define EXPECT(c)                                                   \
  do {                                                              \
    if (!(c)) {                                                     \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);            \
      failures++;                                                   \
    }                                                               \
  } while (0)

static void CheckPlan() {
  const uint32_t rays[] = {1u, 37u, 63u, 64u, 65u, 200u, 4096u, 1u << 20, 0x7FFFFFFFu};
  const uint32_t samples[] = {1u, 2u, 63u, 64u, 65u, 130u, 4096u, 65535u};
  const uint32_t bounds[] = {1u, 7u, 64u, 100u, 4096u, 1u << 24, 0x7FFFFFFFu, 0xFFFFFFFFu};
  for (uint32_t n : rays)
    for (uint32_t k : samples)
      for (uint32_t b : bounds) {
        const RadiancePlan r = PlanRadiance(100u, 1, kFeatXform | kFeatMedium, 8, n, k, b, 256);
        const uint64_t bound = b < 0x7FFFFFFFu ? b : 0x7FFFFFFFu;
        EXPECT(r.q.ok && r.q.threaded && r.q.variant == 1);
        EXPECT(r.rays_per_launch >= 1u && r.per_launch >= 1u && r.ray_launches >= 1u && r.launches >= 1u);
        EXPECT((uint64_t)r.rays_per_launch * r.per_launch <= bound);
        // by sample ranges first: rays are split only where one sample of every ray is too many
        EXPECT(r.ray_launches == 1u || r.per_launch == 1u);
        EXPECT(r.ray_launches == 1u ? r.rays_per_launch == n : (uint64_t)n > bound);
        // no shorter ranges than the bound needs
        EXPECT(r.launches == 1u || (uint64_t)r.rays_per_launch * (r.per_launch + 1u) > bound);
        const bool small = (uint64_t)n * k <= 300000ull && (uint64_t)r.ray_launches * r.launches <= 300000ull;
        std::vector<uint8_t> seen(small ? (size_t)n * k : 0, 0);
        uint64_t total = 0;
        const uint32_t as[] = {0u, r.ray_launches / 2u, r.ray_launches - 1u}, bs[] = {0u, r.launches / 2u, r.launches - 1u};
        if (small) {
          for (uint32_t a = 0; a < r.ray_launches; a++) {
            uint32_t next_s = 0;
            for (uint32_t s = 0; s < r.launches; s++) {
              const RadianceLaunch l = RadianceLaunchAt(r, n, k, a, s);
              EXPECT(l.rays >= 1u && l.k >= 1u && (uint64_t)l.rays * l.k <= bound);
              EXPECT(l.s0 == next_s);  // a ray's sample ranges in increasing order, without a gap
              next_s = l.s0 + l.k;
              const uint32_t items = l.rays * l.k;
              const Magic m = MakeMagic(l.k);
              for (uint32_t w = 0; w < items; w++) {
                uint32_t ray, smp;
                RadianceItem(w, l.k, l.s0, &ray, &smp);
                EXPECT(ray == (uint32_t)(((uint64_t)w * m.m) >> m.s));  // the kernel's division
                const size_t at = (size_t)(l.ray0 + ray) * k + smp;
                EXPECT(l.ray0 + ray < n && smp < k && seen[at] == 0);
                if (l.ray0 + ray < n && smp < k) seen[at]++;
              }
              total += items;
              // the waves' blocks: every item in exactly one, within the grid
              for (bool refill : {false, true}) {
                const uint32_t wi = RadianceWaveItems(items, refill);
                EXPECT(wi % 64u == 0u && wi >= 64u && wi <= 4096u && (refill || wi == 64u));
                const uint32_t grid = RadianceGrid(items, wi, 256u);
                const uint64_t waves = (uint64_t)grid * 4u;
                EXPECT(waves * wi >= items && (waves - 4u) * wi < items);  // whole workgroups, none without an item
                EXPECT(waves * wi < ((uint64_t)1 << 32));  // the kernel's 32-bit block start
              }
            }
            EXPECT(next_s == k);
          }
          EXPECT(total == (uint64_t)n * k);
          for (uint8_t c : seen) EXPECT(c == 1);
        } else {
          for (uint32_t a : as)
            for (uint32_t s : bs) {
              const RadianceLaunch l = RadianceLaunchAt(r, n, k, a, s);
              EXPECT(l.rays >= 1u && l.k >= 1u && (uint64_t)l.rays * l.k <= bound && l.ray0 + l.rays <= n && l.s0 + l.k <= k);
              const uint32_t items = l.rays * l.k, wi = RadianceWaveItems(items, true);
              EXPECT((uint64_t)RadianceGrid(items, wi, 256u) * 4u * wi < ((uint64_t)1 << 32));
            }
          EXPECT((uint64_t)(r.ray_launches - 1u) * r.rays_per_launch < n && (uint64_t)r.ray_launches * r.rays_per_launch >= n);
          EXPECT((uint64_t)(r.launches - 1u) * r.per_launch < k && (uint64_t)r.launches * r.per_launch >= k);
        }
      }
  // both kinds of split at once, and neither
  const RadiancePlan both = PlanRadiance(0u, 1, kFeatAll, 8, 200u, 130u, 64u, 256);
  EXPECT(both.ray_launches == 4u && both.rays_per_launch == 64u && both.per_launch == 1u && both.launches == 130u);
  EXPECT(!both.q.threaded && both.q.variant == -1 && both.q.ok);
  const RadiancePlan samples_only = PlanRadiance(100u, 1, kFeatAll, 8, 37u, 130u, 100u, 256);
  EXPECT(samples_only.ray_launches == 1u && samples_only.per_launch == 2u && samples_only.launches == 65u);
  const RadiancePlan whole = PlanRadiance(100u, 1, kFeatAll, 8, 4096u, 4096u, kRadianceItemsDefault, 256);
  EXPECT(whole.ray_launches == 1u && whole.launches == 1u && whole.per_launch == 4096u);
  EXPECT(!PlanRadiance(0u, 4, kFeatAll, kTraversalStack + 1, 10u, 4u, 100u, 256).q.ok);
}

static uint32_t Bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
static float FromBits(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// 130 samples whose float sum depends on the order (large and small terms, cancellations), with their ray counts in
// word 3: one pass, then every split into ranges of 1, 2, 7, 64, 65 and 129 samples continuing the running answer.
static void CheckOrderedSum() {
  const uint32_t k = 130;
  std::vector<float> slots((size_t)kRadianceSlotWords * k);
  uint32_t x = 12345u;
  uint32_t want_rays = 0;
  for (uint32_t s = 0; s < k; s++) {
    for (int c = 0; c < 3; c++) {
      x = x * 1664525u + 1013904223u;
      const float mag = std::ldexp(1.0f + (float)(x >> 9) * 0x1p-23f, (int)((x >> 3) % 40u) - 20);
      slots[(size_t)kRadianceSlotWords * s + c] = (s % 5u == 4u) ? -mag : mag;
    }
    slots[(size_t)kRadianceSlotWords * s + 3] = FromBits(1u + s % 50u);
    want_rays += 1u + s % 50u;
  }
  float one[3] = {0.0f, 0.0f, 0.0f};
  uint32_t one_rays = 0;
  RadianceSum(slots.data(), k, one, &one_rays);
  EXPECT(one_rays == want_rays);
  // the order matters for these values: the reversed sum differs
  float rev[3] = {0.0f, 0.0f, 0.0f};
  for (uint32_t s = k; s-- > 0;)
    for (int c = 0; c < 3; c++) rev[c] = rev[c] + slots[(size_t)kRadianceSlotWords * s + c];
  EXPECT(Bits(rev[0]) != Bits(one[0]) || Bits(rev[1]) != Bits(one[1]) || Bits(rev[2]) != Bits(one[2]));
  // and it is the plain left-to-right sum
  float plain[3] = {0.0f, 0.0f, 0.0f};
  for (uint32_t s = 0; s < k; s++)
    for (int c = 0; c < 3; c++) plain[c] = plain[c] + slots[(size_t)kRadianceSlotWords * s + c];
  for (int c = 0; c < 3; c++) EXPECT(Bits(plain[c]) == Bits(one[c]));
  for (uint32_t step : {1u, 2u, 7u, 64u, 65u, 129u}) {
    float run[3] = {0.0f, 0.0f, 0.0f};
    uint32_t run_rays = 0;
    for (uint32_t s0 = 0; s0 < k; s0 += step)
      RadianceSum(slots.data() + (size_t)kRadianceSlotWords * s0, step < k - s0 ? step : k - s0, run, &run_rays);
    for (int c = 0; c < 3; c++) EXPECT(Bits(run[c]) == Bits(one[c]));
    EXPECT(run_rays == want_rays);
  }
}

static void CheckRule() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const float good[8] = {1.0f, 2.0f, 3.0f, FLT_MAX, 0.0f, 0.0f, -1.0f, 0.5f};
  EXPECT(RadianceRayValid(good) && QueryRayValid(good));
  const float vals[] = {nan, inf, -inf, 0.0f, -0.0f, 0.001f, 0.0010000002f, 1.0f, 2.0f, -1.0f, 0x1p-21f, 0x1p-20f, 0x1p20f,
                        0x1p21f, 0x1p64f, 0x1.000002p64f, FLT_MAX, -FLT_MAX, 1.0000001f};
  int valid = 0, invalid = 0;
  for (int slot = 0; slot < 8; slot++)
    for (float v : vals) {
      float r[8];
      std::memcpy(r, good, sizeof r);
      r[slot] = v;
      EXPECT(RadianceRayValid(r) == QueryRayValid(r));
      (QueryRayValid(r) ? valid : invalid)++;
    }
  EXPECT(valid >= 30 && invalid >= 30);
  float zero[8];
  std::memcpy(zero, good, sizeof zero);
  zero[6] = 0.0f;
  EXPECT(!RadianceRayValid(zero));
  // the stream words
  const uint32_t words[6] = {5u, 6u, 7u, 8u, 9u, 10u};
  uint32_t pw = 0, fw = 0;
  RadianceStream(words, 100u, 2u, &pw, &fw);
  EXPECT(pw == 9u && fw == 10u);
  RadianceStream(nullptr, 100u, 2u, &pw, &fw);
  EXPECT(pw == 102u && fw == kRadianceFrame0 && kRadianceFrame0 == 0x40000000u && kRadianceInvalid == 0xFFFFFFFFu);
  EXPECT(RadianceFrameFits(kRadianceFrame0, 65535u) && RadianceFrameFits(0xFFFFFFFFu, 1u) && !RadianceFrameFits(0xFFFFFFFFu, 2u));
  EXPECT(RadianceFrameFits(0xFFFF0001u, 65535u) && !RadianceFrameFits(0xFFFF0002u, 65535u) && RadianceFrameFits(0u, 65535u));
  // the arguments
  EXPECT(RadianceArgsValid(1, 0, 0u) && RadianceArgsValid(65535, 65535, 8u));
  EXPECT(!RadianceArgsValid(0, 0, 0u) && !RadianceArgsValid(65536, 0, 0u) && !RadianceArgsValid(-1, 0, 0u));
  EXPECT(!RadianceArgsValid(1, -1, 0u) && !RadianceArgsValid(1, 65536, 0u) && !RadianceArgsValid(1, 0, 9u));
  // the item map: the sample fastest
  uint32_t ray = 0, smp = 0;
  RadianceItem(0u, 5u, 10u, &ray, &smp);
  EXPECT(ray == 0u && smp == 10u);
  RadianceItem(4u, 5u, 10u, &ray, &smp);
  EXPECT(ray == 0u && smp == 14u);
  RadianceItem(5u, 5u, 10u, &ray, &smp);
  EXPECT(ray == 1u && smp == 10u);
}

int main() {
  CheckPlan();
  CheckOrderedSum();
  CheckRule();
  if (failures) return 1;
  std::printf("radiance host ok\n");
  return 0;
}
