// launch_plan.h — the render launch planner: the integer arithmetic between "render n frames" and a
// kernel launch (magic divisors, tile geometry, frames per launch, the chunk schedule, item counts).
// Host only, no HIP call and no tracer: tests/cpp/launch_plan_host.cpp runs it without a GPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "query.h"
#include "rt2_layout.h"

namespace rt2 {

inline Magic MakeMagic(uint32_t d) {  // rt2_layout.h Magic: floor(n / d) for n < 2^31
  uint32_t l = 0;
  while ((1ull << l) < (uint64_t)d) l++;
  const uint64_t m = ((1ull << (31 + l)) + d - 1) / d;
  return Magic{(uint32_t)m, 31 + l};
}

// Work tiles of 64 pixels: 8x8, or as tall as a row band narrower than 8 rows (16x4, 32x2, 64x1)
// so that a wave's pixels stay in one band (neighbouring pixels, coherent primary rays).
// band_h: the band height of the launch (RenderParams::band_h, the image height when unpartitioned).
struct TileGeometry {
  uint32_t tile_shift;
  int tiles_x;
  uint32_t tile_items;
};
inline TileGeometry PlanTiles(int width, int local_rows, int band_h, int world) {
  const int tile_rows = world > 1 && band_h < 8 ? (band_h >= 4 ? 4 : band_h >= 2 ? 2 : 1) : 8;
  TileGeometry g;
  g.tile_shift = tile_rows == 8 ? 3u : tile_rows == 4 ? 4u : tile_rows == 2 ? 5u : 6u;
  g.tiles_x = (width + (1 << g.tile_shift) - 1) >> g.tile_shift;
  g.tile_items = (uint32_t)g.tiles_x * (uint32_t)((local_rows + tile_rows - 1) / tile_rows) * 64u;
  return g;
}

// The sample buffer holds whole octets of frames (rt2_layout.h kOctet).
inline size_t SampleOctets(size_t frames) { return (frames + kOctet - 1) / kOctet * kOctet; }

// Frames per launch: the caller's launch_frames (0: all n_frames), bounded by the sample-buffer budget
// (each of the two slots gets half the budget, so both together stay within it; frame_bytes = one frame
// of samples) and, with frame tiles, by the items (64-frame groups x 64 x local pixels) staying below 2^31.
inline int FramesPerLaunch(int launch_frames, int n_frames, size_t sample_budget, size_t frame_bytes, bool frame_tiles,
                           uint32_t local_pixels) {
  int per_launch = launch_frames > 0 ? std::min(launch_frames, n_frames) : n_frames;
  const size_t budget_frames = std::max<size_t>(1, sample_budget / 2 / frame_bytes);
  per_launch = (int)std::min<size_t>((size_t)per_launch, budget_frames < kOctet ? budget_frames : budget_frames - budget_frames % kOctet);
  if (frame_tiles) {
    const size_t groups = std::max<size_t>(1, (size_t)0x7FFFFFFF / (64u * (size_t)local_pixels));
    per_launch = (int)std::min<size_t>((size_t)per_launch, groups * 64u);
  }
  return per_launch;
}

struct ChunkSettings {
  bool frame_tiles;    // items = one pixel x 64 short chunks per wave
  int frame_tile_len;  // most frames per chunk in frame-tile mode
  int work_split;      // work left split into >= k items per lane (0: one chunk)
  int chunk_max;       // longest chunk (frames)
  bool chunk_align;    // chunks of >= kOctet frames: multiples of 4 frames
};

// Frame chunks of one launch: frames [fb, fb + n) cut into chunks, every pixel's chunk c one work
// item (chunk-major). A chunk starting with R frames left holds about R * T / (k * L) frames (T =
// items per chunk, L = resident lanes, k = work_split), at least 1 and at most chunk_max: early
// items are long (few item setups per sample) and the last ones short, so the launch's tail — the
// time in which lanes run out of work while others finish their item — stays short. k = 0: one
// chunk (each pixel's frames in one item). Appends the table (first frame, stratum) per chunk and
// the sentinel to `tab`; returns the number of chunks and the first chunk's length.
inline void ChunkSchedule(const ChunkSettings& t, int fb, int n, uint32_t tile_items, int64_t lanes, int sq,
                          std::vector<uint32_t>& tab, uint32_t* n_chunks, int* first_len) {
  const size_t start = tab.size();
  // items must stay below 2^31 (kernel index arithmetic): shortest chunk that allows it
  const int64_t max_chunks = std::max<int64_t>(1, (int64_t)0x7FFFFFFF / tile_items);
  const int lo = (int)std::max<int64_t>(1, ((int64_t)n + max_chunks - 1) / max_chunks);
  int first = 0;
  // frame tiles: chunks of up to frame_tile_len frames, as even as the 64-chunk groups allow (the
  // last group is padded with empty chunks, whose lanes fetch again)
  int ft_len = 1;
  if (t.frame_tiles) {
    const int groups = (n + 64 * t.frame_tile_len - 1) / (64 * t.frame_tile_len);
    ft_len = (n + 64 * groups - 1) / (64 * groups);
  }
  for (int s = 0; s < n;) {
    int len = n - s;
    if (t.frame_tiles) {
      len = ft_len;  // frame tiles: short chunks of one pixel (RenderParams::frame_tiles)
    } else if (t.work_split > 0) {
      const double want = (double)(n - s) * (double)tile_items / ((double)t.work_split * (double)lanes);
      len = (int)std::min<double>(want, (double)t.chunk_max);
    }
    // long chunks start on a 4-frame group of the sample octets (the 8-wave kernels stage samples
    // by 4 frames; whole octets would cut a 15-frame chunk to 8)
    if (t.chunk_align && len >= (int)kOctet) len -= len % 4;
    if (!t.frame_tiles) len = std::max(len, lo);
    len = std::min({len, n - s, kChunkMaxFrames});
    const uint32_t f = (uint32_t)(fb + s), usq = (uint32_t)sq;
    tab.push_back(f);
    tab.push_back((f % usq) | (((f / usq) % usq) << 16));  // RayTracer.cpp:59-60
    if (s == 0) first = len;
    s += len;
  }
  if (t.frame_tiles) {  // padding chunks up to a multiple of 64 (empty: first frame = the launch end)
    while (((tab.size() - start) / 2) % 64 != 0) {
      tab.push_back((uint32_t)(fb + n));
      tab.push_back(0u);
    }
  }
  tab.push_back((uint32_t)(fb + n));
  tab.push_back(0u);
  *n_chunks = (uint32_t)((tab.size() - start) / 2 - 1);
  *first_len = first;
}

// Per-launch item fields: the work items of n_chunks chunks (frame tiles: 64-chunk groups of one pixel each),
// the reservation divisor (half of the left work / waves) and the grid of `block`-lane workgroups that
// `resident` lanes, or the items if fewer, fill.
struct LaunchItems {
  uint32_t n_items, frame_tile, batch_div;
  int grid;
};
inline LaunchItems PlanItems(uint32_t n_chunks, uint32_t tile_items, bool frame_tiles, uint32_t local_pixels,
                             int64_t resident, int block) {
  LaunchItems it;
  it.frame_tile = frame_tiles ? 64u * local_pixels : 0u;
  it.n_items = frame_tiles ? (n_chunks / 64u) * it.frame_tile : n_chunks * tile_items;
  it.batch_div = (uint32_t)std::max<int64_t>(1, (resident / 64) * 2);
  it.grid = std::max((int)std::min<int64_t>(resident, (int64_t)it.n_items) / block, 1);
  return it;
}

// A ray-query launch (rt2.h "Ray queries"; render.hip query_kernel) over n rays, 0 < n < 2^31, from the scene's
// facts: lin_len, the steps of its threaded program (0: none, or switched off); variant and variant_features,
// the instantiation of its feature set (RenderVariant, RenderVariantFeatures); stack_depth, the entries its stack
// walk needs; block, the workgroup's lanes. The threaded program wherever there is one, else the stack walk, which
// has one instantiation (variant -1) and cannot serve a scene whose stack is deeper than the kernel's (ok false:
// the call is refused). grid: workgroups over n rounded up to whole waves. lds_dynamic: what the launch asks for
// (the stack walk's per-lane stacks); lds_static: the threaded kernels' box-boundary candidate planes (the
// instantiations with media and no spheres, render.hip BoxPair).
struct QueryPlan {
  bool ok, threaded;
  int variant;
  uint32_t grid;
  size_t lds_dynamic, lds_static;
};
inline QueryPlan PlanQuery(uint32_t lin_len, int variant, uint32_t variant_features, int stack_depth, uint32_t n,
                           int block) {
  QueryPlan q;
  q.threaded = lin_len != 0;
  q.ok = q.threaded || stack_depth <= kTraversalStack;
  q.variant = q.threaded ? variant : -1;
  q.grid = QueryGrid(n, (uint32_t)block);
  q.lds_dynamic = q.threaded ? 0 : (size_t)stack_depth * (size_t)block * 4;
  const bool planes = q.threaded && (variant_features & kFeatMedium) != 0u && (variant_features & kFeatSphere) == 0u;
  q.lds_static = planes ? (size_t)(block / 64) * kBoundaryAAMax * 64 * 4 : 0;
  return q;
}

// An ambient-occlusion call (rt2.h "Ambient occlusion"; render.hip ambient_kernel) over `points` points, 0 <
// points < 2^31, of `samples` samples each, 1 <= samples <= 65535. Work items are (point, sample): a launch takes
// per_launch consecutive samples of every point, as many as keep points x per_launch below 2^31, and the call is
// `launches` launches over consecutive sample ranges (the last one takes last samples). The counts are integer
// sums, so the split does not show in the result. The walk, variant and LDS: as PlanQuery over one launch's items.
struct AmbientPlan {
  QueryPlan q;  // of a launch of per_launch samples
  uint32_t per_launch, launches, last;
};
inline AmbientPlan PlanAmbient(uint32_t lin_len, int variant, uint32_t variant_features, int stack_depth,
                               uint32_t points, uint32_t samples, int block) {
  AmbientPlan a;
  a.per_launch = std::min<uint32_t>(samples, 0x7FFFFFFFu / points);
  a.launches = (samples + a.per_launch - 1u) / a.per_launch;
  a.last = samples - (a.launches - 1u) * a.per_launch;
  a.q = PlanQuery(lin_len, variant, variant_features, stack_depth, points * a.per_launch, block);
  return a;
}

// A radiance call (rt2.h "Radiance queries"; render.hip radiance_kernel) over `rays` rays, 0 < rays < 2^31, of
// `samples` samples each, 1 <= samples <= 65535. Work items are (ray, sample), one result slot each. A launch
// holds at most min(items_max, 2^31 - 1) items (items_max >= 1: RT2_RADIANCE_ITEMS, the slot buffer's bound): the
// call is split by sample ranges first (per_launch consecutive samples of every ray), and where one sample of
// every ray is still too many, by ray ranges (rays_per_launch consecutive rays). Launch (a, b), a over the ray
// ranges and b over the sample ranges, b fastest: each ray's sample ranges run in increasing order, which the
// ordered sum needs. Every wave owns wave_items consecutive items of its launch (a multiple of 64; 64 without
// refill: one item per lane); with refill the blocks grow with the launch so that about kRadianceWaves waves
// share it, up to 64 items per lane.
// (2^24 items are 256 MiB of 16-byte slots, float3 plus the ray count; 192 MiB would be 12-byte slots without it)
constexpr uint32_t kRadianceItemsDefault = 1u << 24;
// The most RT2_RADIANCE_ITEMS is taken for: 2^28 items, a slot buffer of 4 GiB; a larger value is read as this one.
constexpr uint32_t kRadianceItemsEnvMax = 1u << 28;
constexpr uint32_t kRadianceWaves = 8192;
struct RadiancePlan {
  QueryPlan q;  // of the first launch (the largest)
  uint32_t rays_per_launch, ray_launches, per_launch, launches;
};
struct RadianceLaunch {
  uint32_t ray0, rays, s0, k;
};
inline RadiancePlan PlanRadiance(uint32_t lin_len, int variant, uint32_t variant_features, int stack_depth,
                                 uint32_t rays, uint32_t samples, uint32_t items_max, int block) {
  RadiancePlan r;
  const uint32_t bound = std::min<uint32_t>(std::max<uint32_t>(items_max, 1u), 0x7FFFFFFFu);
  r.rays_per_launch = std::min(rays, bound);
  r.ray_launches = (rays + r.rays_per_launch - 1u) / r.rays_per_launch;
  r.per_launch = std::min<uint32_t>(samples, std::max<uint32_t>(1u, bound / r.rays_per_launch));
  r.launches = (samples + r.per_launch - 1u) / r.per_launch;
  r.q = PlanQuery(lin_len, variant, variant_features, stack_depth, r.rays_per_launch * r.per_launch, block);
  return r;
}
inline RadianceLaunch RadianceLaunchAt(const RadiancePlan& r, uint32_t rays, uint32_t samples, uint32_t a, uint32_t b) {
  RadianceLaunch l;
  l.ray0 = a * r.rays_per_launch;
  l.rays = std::min(r.rays_per_launch, rays - l.ray0);
  l.s0 = b * r.per_launch;
  l.k = std::min(r.per_launch, samples - l.s0);
  return l;
}
inline uint32_t RadianceWaveItems(uint32_t items, bool refill) {
  if (!refill) return 64u;
  const uint32_t per_lane = (items + 64u * kRadianceWaves - 1u) / (64u * kRadianceWaves);
  return 64u * std::min<uint32_t>(std::max<uint32_t>(per_lane, 1u), 64u);
}
// The launch's workgroups of `block` lanes: one wave per block of wave_items items.
inline uint32_t RadianceGrid(uint32_t items, uint32_t wave_items, uint32_t block) {
  const uint32_t waves = (items + wave_items - 1u) / wave_items;
  return (waves * 64u + block - 1u) / block;
}

}  // namespace rt2
