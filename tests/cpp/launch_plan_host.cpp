// launch_plan_host.cpp — the render launch planner (raytrace2_amd/csrc/launch_plan.h) on the host: the magic
// divisors against plain division, the chunk schedule's invariants over a grid of launches, a few schedules
// pinned word for word (recorded from the schedule function as it stood inside capi.cpp, before it moved to
// the header), and literal tile shapes, frames-per-launch bounds and item counts. A stand-alone program:
// tests/test_launch_plan_host.py builds it plain and with the host sanitizers. Exit status 0: all passed.
#include <cstdio>
#include <cstdlib>

#include "launch_plan.h"

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

// ---- MakeMagic: (n * m) >> s == n / d for every n < 2^31 ----
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t Rand31() {  // xorshift64*
  g_rng ^= g_rng >> 12;
  g_rng ^= g_rng << 25;
  g_rng ^= g_rng >> 27;
  return (uint32_t)((g_rng * 0x2545F4914F6CDD1Dull) >> 33);
}
static void CheckMagic(uint32_t d) {
  const Magic k = MakeMagic(d);
  CHECK(k.s >= 31 && k.s < 63, "d %u: shift %u", d, k.s);
  const auto one = [&](uint32_t n) {
    CHECK((uint32_t)(((uint64_t)n * k.m) >> k.s) == n / d, "d %u n %u: m %u s %u", d, n, k.m, k.s);
  };
  const uint64_t edge[] = {0, 1, (uint64_t)d - 1, d, (uint64_t)d + 1, 2 * (uint64_t)d - 1, 0x7FFFFFFF};
  for (uint64_t n : edge)
    if (n <= 0x7FFFFFFFull) one((uint32_t)n);
  for (int i = 0; i < 64; i++) one(Rand31());
}
static void TestMagic() {
  for (uint32_t d = 1; d <= 4096; d++) CheckMagic(d);
  for (int k = 0; k <= 30; k++) {
    const uint32_t p = 1u << k;
    if (p > 1) CheckMagic(p - 1);
    CheckMagic(p);
    CheckMagic(p + 1);
  }
  CheckMagic(0x7FFFFFFFu);
}

// ---- ChunkSchedule: invariants ----
static void CheckSchedule(const ChunkSettings& c, int fb, int n, uint32_t tile_items, int64_t lanes, int sq) {
  std::vector<uint32_t> tab{0xDEADu, 0xBEEFu};  // appended to: what `tab` holds stays
  uint32_t n_chunks = 0;
  int first_len = 0;
  ChunkSchedule(c, fb, n, tile_items, lanes, sq, tab, &n_chunks, &first_len);
#define WHERE "ft %d/%d split %d max %d align %d fb %d n %d items %u lanes %lld sq %d", (int)c.frame_tiles, \
              c.frame_tile_len, c.work_split, c.chunk_max, (int)c.chunk_align, fb, n, tile_items, (long long)lanes, sq
  CHECK(tab[0] == 0xDEADu && tab[1] == 0xBEEFu, WHERE);
  CHECK(tab.size() == 2 + 2 * ((size_t)n_chunks + 1), WHERE);
  if (tab.size() != 2 + 2 * ((size_t)n_chunks + 1) || n_chunks == 0) return;
  const uint32_t* t = tab.data() + 2;
  const uint32_t end = (uint32_t)(fb + n), usq = (uint32_t)sq;
  // the sentinel
  CHECK(t[2 * n_chunks] == end && t[2 * n_chunks + 1] == 0u, WHERE);
  // the 2^31 floor: the shortest chunk that keeps chunks * tile_items below 2^31
  const int64_t max_chunks = std::max<int64_t>(1, (int64_t)0x7FFFFFFF / tile_items);
  const int lo = (int)std::max<int64_t>(1, ((int64_t)n + max_chunks - 1) / max_chunks);
  // the longest chunk the settings allow: frame tiles cut by frame_tile_len; chunk_max bounds the chunks that
  // work_split sizes (work_split 0 asks for one chunk, which only kChunkMaxFrames cuts)
  int cap = c.frame_tiles ? c.frame_tile_len : c.work_split > 0 ? std::min(c.chunk_max, kChunkMaxFrames) : kChunkMaxFrames;
  if (!c.frame_tiles) cap = std::max(cap, std::min(lo, kChunkMaxFrames));  // ... except where the floor forces it longer
  uint32_t real = 0;  // chunks that hold frames (frame tiles pad with empty ones)
  while (real < n_chunks && t[2 * real] < end) real++;
  CHECK(real >= 1 && t[0] == (uint32_t)fb, WHERE);
  int sum = 0;
  for (uint32_t i = 0; i < real; i++) {
    const uint32_t f = t[2 * i];
    const int len = (int)(t[2 * i + 2] - f);  // the next chunk's first frame, the first padding chunk's or the sentinel's
    CHECK(t[2 * i + 2] > f, WHERE);
    CHECK(len >= 1 && len <= cap, WHERE);
    CHECK(f == (uint32_t)(fb + sum), WHERE);
    CHECK(t[2 * i + 1] == ((f % usq) | (((f / usq) % usq) << 16)), WHERE);
    if (c.chunk_align && len >= (int)kOctet) CHECK(len % 4 == 0 || sum + len == n, WHERE);
    if (i == 0) CHECK(first_len == len, WHERE);
    sum += len;
  }
  CHECK(sum == n, WHERE);
  for (uint32_t i = real; i < n_chunks; i++) CHECK(t[2 * i] == end && t[2 * i + 1] == 0u, WHERE);
  if (c.frame_tiles) {
    CHECK(n_chunks % 64 == 0 && n_chunks - real < 64, WHERE);
  } else {
    CHECK(real == n_chunks, WHERE);
    // Work items stay below 2^31 wherever a chunk of kChunkMaxFrames frames (the kernel's 11-bit counter) can
    // be as long as the floor asks. Past that (n = 2049 frames of 0x7FFFFFC0 items: more than 48 TiB of
    // samples, which no launch gets: FramesPerLaunch's budget bound comes first) the chunks are cut at
    // kChunkMaxFrames, as the schedule always has.
    if (lo <= kChunkMaxFrames) CHECK((uint64_t)n_chunks * tile_items <= 0x7FFFFFFFull, WHERE);
    else CHECK(first_len == kChunkMaxFrames, WHERE);
  }
#undef WHERE
}

static void TestScheduleGrid() {
  const int ns[] = {1, 7, 8, 9, 15, 64, 65, 1000, 2049}, fbs[] = {0, 5, 1000}, sqs[] = {1, 4, 31}, splits[] = {0, 1, 4};
  const int maxes[] = {1, 64, 4096};
  const uint32_t items[] = {64u, 1u << 20, 0x7FFFFFC0u};
  const int64_t lanes[] = {256, 256 * 8 * 256};
  const int ft_lens[] = {1, 8, 64}, ft_ns[] = {1, 63, 64, 65, 513};
  for (int fb : fbs)
    for (int sq : sqs)
      for (int ws : splits)
        for (int cm : maxes)
          for (int al = 0; al < 2; al++)
            for (uint32_t ti : items)
              for (int64_t ln : lanes) {
                for (int n : ns) CheckSchedule(ChunkSettings{false, 8, ws, cm, al != 0}, fb, n, ti, ln, sq);
                for (int ftl : ft_lens)
                  for (int n : ft_ns) CheckSchedule(ChunkSettings{true, ftl, ws, cm, al != 0}, fb, n, ti, ln, sq);
              }
}

// ---- ChunkSchedule: pinned tables ----
struct Pinned {
  ChunkSettings c;
  int fb, n;
  uint32_t tile_items;
  int64_t lanes;
  int sq;
  uint32_t n_chunks;
  int first_len;
  std::vector<uint32_t> tab;
};
static void TestPinned() {
  const Pinned pinned[] = {
    // the headline shape: 1024^2 pixels, 1000 frames, work_split 4
    {{false, 8, 4, 64, true}, 0, 1000, 0x100000u, 524288, 4, 22u, 64,
     {0u, 0u, 64u, 0u, 128u, 0u, 192u, 0u, 256u, 0u, 320u, 0u,
      384u, 0u, 448u, 0u, 512u, 0u, 576u, 0u, 640u, 0u, 704u, 0u,
      768u, 0u, 832u, 0u, 896u, 0u, 948u, 0x10000u, 972u, 0x30000u, 984u, 0x20000u,
      992u, 0u, 996u, 0x10000u, 998u, 0x10002u, 999u, 0x10003u, 1000u, 0u}},
    // work_split 0: each pixel's frames in one item, cut only by the 4-frame alignment
    {{false, 8, 0, 64, true}, 5, 65, 0x100000u, 524288, 4, 2u, 64,
     {5u, 0x10001u, 69u, 0x10001u, 70u, 0u}},
    // chunk_align off
    {{false, 8, 4, 4096, false}, 1000, 65, 0x100000u, 524288, 31, 8u, 32,
     {1000u, 0x10008u, 1032u, 0x20009u, 1048u, 0x20019u, 1056u, 0x30002u, 1060u, 0x30006u, 1062u, 0x30008u,
      1063u, 0x30009u, 1064u, 0x3000Au, 1065u, 0u}},
    // frame tiles, 33 chunks of <= 2 frames padded to 64
    {{true, 8, 4, 64, true}, 5, 65, 0x40u, 256, 4, 64u, 2,
     {5u, 0x10001u, 7u, 0x10003u, 9u, 0x20001u, 11u, 0x20003u, 13u, 0x30001u, 15u, 0x30003u,
      17u, 1u, 19u, 3u, 21u, 0x10001u, 23u, 0x10003u, 25u, 0x20001u, 27u, 0x20003u,
      29u, 0x30001u, 31u, 0x30003u, 33u, 1u, 35u, 3u, 37u, 0x10001u, 39u, 0x10003u,
      41u, 0x20001u, 43u, 0x20003u, 45u, 0x30001u, 47u, 0x30003u, 49u, 1u, 51u, 3u,
      53u, 0x10001u, 55u, 0x10003u, 57u, 0x20001u, 59u, 0x20003u, 61u, 0x30001u, 63u, 0x30003u,
      65u, 1u, 67u, 3u, 69u, 0x10001u, 70u, 0u, 70u, 0u, 70u, 0u,
      70u, 0u, 70u, 0u, 70u, 0u, 70u, 0u, 70u, 0u, 70u, 0u,
      70u, 0u, 70u, 0u, 70u, 0u, 70u, 0u, 70u, 0u, 70u, 0u,
      70u, 0u, 70u, 0u, 70u, 0u, 70u, 0u, 70u, 0u, 70u, 0u,
      70u, 0u, 70u, 0u, 70u, 0u, 70u, 0u, 70u, 0u, 70u, 0u,
      70u, 0u, 70u, 0u, 70u, 0u, 70u, 0u, 70u, 0u}},
    // the 2^31 floor: at most 7 chunks of 2^28 items, so 15 frames go in chunks of 3
    {{false, 8, 4, 1, true}, 0, 15, 0x10000000u, 524288, 4, 5u, 3,
     {0u, 0u, 3u, 3u, 6u, 0x10002u, 9u, 0x20001u, 12u, 0x30000u, 15u, 0u}},
    // n = 1
    {{false, 8, 4, 64, true}, 1000, 1, 0x40u, 256, 31, 1u, 1,
     {1000u, 0x10008u, 1001u, 0u}},
  };
  int k = 0;
  for (const Pinned& p : pinned) {
    std::vector<uint32_t> tab;
    uint32_t n_chunks = 0;
    int first_len = 0;
    ChunkSchedule(p.c, p.fb, p.n, p.tile_items, p.lanes, p.sq, tab, &n_chunks, &first_len);
    CHECK(tab == p.tab && n_chunks == p.n_chunks && first_len == p.first_len, "pinned table %d", k);
    k++;
  }
}

// ---- tile geometry, frames per launch, items ----
static void TestTiles() {
  struct Case {
    int band_h, world;
    TileGeometry want;
  };
  // a 1000-pixel-wide image, 100 local rows. band_h is the launch's band height (RenderParams::band_h: callers
  // pass the image height for an unbanded tracer, never 0, which counts as a band narrower than 2 rows)
  const Case cases[] = {{1, 8, {6u, 16, 102400u}}, {2, 8, {5u, 32, 102400u}}, {4, 8, {4u, 63, 100800u}},
                        {8, 8, {3u, 125, 104000u}}, {0, 8, {6u, 16, 102400u}}, {2, 1, {3u, 125, 104000u}}};
  for (const Case& c : cases) {
    const TileGeometry g = PlanTiles(1000, 100, c.band_h, c.world);
    CHECK(g.tile_shift == c.want.tile_shift && g.tiles_x == c.want.tiles_x && g.tile_items == c.want.tile_items,
          "band_h %d world %d: shift %u tiles_x %d items %u", c.band_h, c.world, g.tile_shift, g.tiles_x, g.tile_items);
  }
}

static void TestFramesPerLaunch() {
  const size_t fbytes = 1000 * 12;  // 1000 local pixels
  CHECK(FramesPerLaunch(0, 100, 2 * fbytes * 5, fbytes, false, 1000) == 5, "a budget below one octet");
  CHECK(FramesPerLaunch(0, 100, 0, fbytes, false, 1000) == 1, "no budget: one frame");
  CHECK(FramesPerLaunch(0, 100, 2 * fbytes * 8, fbytes, false, 1000) == 8, "a budget of exactly one octet");
  CHECK(FramesPerLaunch(0, 100, 2 * fbytes * 15, fbytes, false, 1000) == 8, "whole octets");
  CHECK(FramesPerLaunch(0, 100, 2 * fbytes * 1000, fbytes, false, 1000) == 100, "all frames");
  CHECK(FramesPerLaunch(7, 100, 2 * fbytes * 1000, fbytes, false, 1000) == 7, "launch_frames");
  CHECK(FramesPerLaunch(200, 100, 2 * fbytes * 1000, fbytes, false, 1000) == 100, "launch_frames above n_frames");
  // frame tiles: 31 groups of 64 x 64 x 2^20 items stay below 2^31
  const size_t big = (size_t)12 << 20;
  CHECK(FramesPerLaunch(0, 4096, (size_t)1 << 60, big, true, 1u << 20) == 1984, "the frame-tile 2^31 cap");
  CHECK(FramesPerLaunch(0, 4096, (size_t)1 << 60, big, false, 1u << 20) == 4096, "no cap without frame tiles");
  CHECK(SampleOctets(0) == 0 && SampleOctets(1) == 8 && SampleOctets(8) == 8 && SampleOctets(9) == 16, "octets");
}

static void TestItems() {
  LaunchItems it = PlanItems(22, 1u << 20, false, 1u << 20, 524288, 256);
  CHECK(it.n_items == 23068672u && it.frame_tile == 0u && it.batch_div == 16384u && it.grid == 2048, "headline items");
  it = PlanItems(1, 64, false, 64, 524288, 256);
  CHECK(it.n_items == 64u && it.batch_div == 16384u && it.grid == 1, "fewer items than a workgroup");
  it = PlanItems(64, 128, true, 100, 524288, 256);
  CHECK(it.n_items == 6400u && it.frame_tile == 6400u && it.grid == 25, "frame-tile items");
  it = PlanItems(128, 128, true, 100, 32, 256);
  CHECK(it.n_items == 12800u && it.batch_div == 1u && it.grid == 1, "few resident lanes");
}

int main() {
  TestMagic();
  TestScheduleGrid();
  TestPinned();
  TestTiles();
  TestFramesPerLaunch();
  TestItems();
  if (g_failed) {
    fprintf(stderr, "%d checks failed\n", g_failed);
    return 1;
  }
  printf("launch plan ok\n");
  return 0;
}
