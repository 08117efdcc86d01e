// adaptive.hip — the check of adaptive sampling (rt2.h "Adaptive sampling"): which pixels retire, and the
// list of the pixels still active that the next render launches run over. Four kernels on the tracer's
// stream, no atomics anywhere, so the same image gives the same flags, list and scalars every time:
//
//   classify  one thread per local pixel: `over` (adaptive.h AdaptiveOver, double arithmetic, the function
//             the host test runs) from the pixel's sums and its own sample count; one partial per workgroup
//             with the non-finite pixels (ballot + popcount) and the sum of the sample counts.
//   retire    one workgroup per tile of 32 columns x 8 local rows, a wave per 8 x 8 pixels. The tile's rows
//             of `over` flags, with kAdaptiveWindowMax columns on either side, go to LDS; an active pixel
//             stays active iff a flag within its window is set (adaptive.h AdaptiveWindowOver). The new
//             flags come out with the workgroup's count of active pixels and of pixels retired now
//             (ballot + popcount per wave, the four waves added through LDS).
//   scan      one workgroup: the exclusive scan of the workgroups' active counts (each thread sums a
//             contiguous share, thread 0 scans the 256 shares in order), the check's totals, and the
//             padding of the list to a multiple of 64 with width * rows (render.hip: a slot no lane renders).
//   scatter   the retire geometry again: active_list[slot] = local pixel, slot_of[local pixel] = slot, with
//             slot = the workgroup's offset + the active lanes before this one in the workgroup.
//
// List order (it affects speed only, never results): tile-major. Tiles of 32 x 8 pixels in row-major tile
// order; within a tile its four 8 x 8 blocks left to right; within a block row by row. While few pixels
// have retired, 64 consecutive slots (one wave of the render kernel) are therefore an 8 x 8 block or a few
// neighbouring ones, as coherent as the full launch's 8 x 8 work tiles.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "adaptive.h"
#include "kernels.h"

namespace rt2 {
namespace dev {

constexpr int kAdBlock = 256;
constexpr int kAdWaves = kAdBlock / 64;
constexpr int kAdTileW = 32, kAdTileH = 8;  // a workgroup's pixels: four 8 x 8 blocks side by side
constexpr int kAdSpan = kAdTileW + 2 * kAdaptiveWindowMax;  // columns of `over` flags a tile's windows reach

__global__ __launch_bounds__(kAdBlock) void adaptive_classify_kernel(const float* __restrict__ accum,
                                                                     const float* __restrict__ moment2,
                                                                     const uint32_t* __restrict__ counts,
                                                                     uint8_t* __restrict__ over,
                                                                     AdaptivePartial* __restrict__ partials,
                                                                     uint32_t npix, double threshold) {
  __shared__ AdaptivePartial part[kAdWaves];
  const uint32_t i = blockIdx.x * (uint32_t)kAdBlock + threadIdx.x;
  bool bad = false;
  unsigned long long n = 0ull;  // lanes past the image add nothing
  if (i < npix) {
    const float a[3] = {accum[3ull * i], accum[3ull * i + 1], accum[3ull * i + 2]};
    const float q[3] = {moment2[3ull * i], moment2[3ull * i + 1], moment2[3ull * i + 2]};
    const uint32_t np = counts[i];
    const PixelOver o = AdaptiveOver(a, q, np, threshold);
    over[i] = o.over ? 1 : 0;
    bad = !o.finite;
    n = np;
  }
  const uint64_t n_bad = (uint64_t)__popcll(__ballot(bad));
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) n = n + __shfl_xor(n, d, 64);
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) {
    part[wave].nonfinite = n_bad;
    part[wave].samples = n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    AdaptivePartial r = part[0];
    for (int w = 1; w < kAdWaves; w++) {
      r.nonfinite += part[w].nonfinite;
      r.samples += part[w].samples;
    }
    partials[blockIdx.x] = r;
  }
}

// This thread's pixel of the workgroup's tile: false for a lane past the image's edge.
__device__ __forceinline__ bool tile_pixel(int width, int rows, int& x, int& r) {
  const int w = (int)(threadIdx.x >> 6), l = (int)(threadIdx.x & 63u);
  x = (int)blockIdx.x * kAdTileW + w * 8 + (l & 7);
  r = (int)blockIdx.y * kAdTileH + (l >> 3);
  return x < width && r < rows;
}

__global__ __launch_bounds__(kAdBlock) void adaptive_retire_kernel(const uint8_t* __restrict__ over,
                                                                   uint8_t* __restrict__ active,
                                                                   uint2* __restrict__ wg_counts, int width, int rows,
                                                                   int window) {
  __shared__ uint8_t s_over[kAdTileH][kAdSpan];
  __shared__ uint2 s_cnt[kAdWaves];
  const int base = (int)blockIdx.x * kAdTileW - kAdaptiveWindowMax;  // column of s_over[.][0]
  for (int k = (int)threadIdx.x; k < kAdTileH * kAdSpan; k += kAdBlock) {
    const int rr = k / kAdSpan, cc = k - rr * kAdSpan;
    const int col = base + cc, row = (int)blockIdx.y * kAdTileH + rr;
    uint8_t v = 0;
    if (col >= 0 && col < width && row < rows) v = over[(size_t)row * (size_t)width + (size_t)col];
    s_over[rr][cc] = v;
  }
  __syncthreads();
  int x, r;
  bool stays = false, retires = false;
  if (tile_pixel(width, rows, x, r)) {
    const size_t i = (size_t)r * (size_t)width + (size_t)x;
    if (active[i]) {
      stays = AdaptiveWindowOver(s_over[r - (int)blockIdx.y * kAdTileH], base, x, width, window);
      retires = !stays;
      if (retires) active[i] = 0;
    }
  }
  const uint32_t n_stay = (uint32_t)__popcll(__ballot(stays));
  const uint32_t n_ret = (uint32_t)__popcll(__ballot(retires));
  if ((threadIdx.x & 63u) == 0u) s_cnt[threadIdx.x >> 6] = make_uint2(n_stay, n_ret);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint2 c = s_cnt[0];
    for (int w = 1; w < kAdWaves; w++) c.x += s_cnt[w].x, c.y += s_cnt[w].y;
    wg_counts[blockIdx.y * gridDim.x + blockIdx.x] = c;
  }
}

__global__ __launch_bounds__(kAdBlock) void adaptive_scan_kernel(const uint2* __restrict__ wg_counts,
                                                                 uint32_t* __restrict__ wg_offsets, uint32_t n_wg,
                                                                 const AdaptivePartial* __restrict__ partials,
                                                                 uint32_t n_partials, uint32_t* __restrict__ list,
                                                                 uint32_t sentinel, AdaptiveTotals* __restrict__ totals) {
  __shared__ uint32_t s_act[kAdBlock];  // each thread's share, then its exclusive offset
  __shared__ unsigned long long s_ret[kAdBlock], s_bad[kAdBlock], s_smp[kAdBlock];
  __shared__ uint32_t s_total;
  const uint32_t t = threadIdx.x;
  const uint32_t share = (n_wg + (uint32_t)kAdBlock - 1u) / (uint32_t)kAdBlock;
  const uint32_t w0 = t * share < n_wg ? t * share : n_wg, w1 = w0 + share < n_wg ? w0 + share : n_wg;
  uint32_t act = 0;
  unsigned long long ret = 0ull;
  for (uint32_t w = w0; w < w1; w++) {
    act += wg_counts[w].x;
    ret += wg_counts[w].y;
  }
  const uint32_t pshare = (n_partials + (uint32_t)kAdBlock - 1u) / (uint32_t)kAdBlock;
  const uint32_t p0 = t * pshare < n_partials ? t * pshare : n_partials;
  const uint32_t p1 = p0 + pshare < n_partials ? p0 + pshare : n_partials;
  unsigned long long bad = 0ull, smp = 0ull;
  for (uint32_t p = p0; p < p1; p++) {
    bad += partials[p].nonfinite;
    smp += partials[p].samples;
  }
  s_act[t] = act;
  s_ret[t] = ret;
  s_bad[t] = bad;
  s_smp[t] = smp;
  __syncthreads();
  if (t == 0) {
    uint32_t run = 0;
    unsigned long long r = 0ull, b = 0ull, s = 0ull;
    for (int k = 0; k < kAdBlock; k++) {
      const uint32_t c = s_act[k];
      s_act[k] = run;
      run += c;
      r += s_ret[k];
      b += s_bad[k];
      s += s_smp[k];
    }
    s_total = run;
    totals->active = run;
    totals->retired = r;
    totals->nonfinite = b;
    totals->samples = s;
  }
  __syncthreads();
  uint32_t off = s_act[t];
  for (uint32_t w = w0; w < w1; w++) {
    wg_offsets[w] = off;
    off += wg_counts[w].x;
  }
  // the list's padding slots, up to the next multiple of 64 (the list holds sentinel + 64 entries)
  const uint32_t total = s_total;
  if (t < 64u && total + t < ((total + 63u) & ~63u)) list[total + t] = sentinel;
}

__global__ __launch_bounds__(kAdBlock) void adaptive_scatter_kernel(const uint8_t* __restrict__ active,
                                                                    const uint32_t* __restrict__ wg_offsets,
                                                                    uint32_t* __restrict__ list,
                                                                    uint32_t* __restrict__ slot_of, int width,
                                                                    int rows) {
  __shared__ uint32_t s_cnt[kAdWaves];
  int x, r;
  bool on = false;
  uint32_t i = 0;
  if (tile_pixel(width, rows, x, r)) {
    i = (uint32_t)r * (uint32_t)width + (uint32_t)x;
    on = active[i] != 0;
  }
  const unsigned long long mask = __ballot(on);
  const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) s_cnt[wave] = (uint32_t)__popcll(mask);
  __syncthreads();
  if (on) {
    uint32_t slot = wg_offsets[blockIdx.y * gridDim.x + blockIdx.x] + before;
    for (uint32_t w = 0; w < wave; w++) slot += s_cnt[w];
    list[slot] = i;
    slot_of[i] = slot;
  }
}

}  // namespace dev

uint32_t AdaptiveBlocks(uint32_t npix) { return (npix + (uint32_t)dev::kAdBlock - 1u) / (uint32_t)dev::kAdBlock; }
uint32_t AdaptiveTiles(int width, int rows) {
  return (uint32_t)((width + dev::kAdTileW - 1) / dev::kAdTileW) * (uint32_t)((rows + dev::kAdTileH - 1) / dev::kAdTileH);
}

// One check over width x rows local pixels (> 0). Buffers: over, active [pixels]; list [pixels + 64];
// slot_of [pixels]; wg_counts, wg_offsets [AdaptiveTiles]; partials [AdaptiveBlocks]; totals [1].
hipError_t LaunchAdaptiveCheck(const float* accum, const float* moment2, const uint32_t* counts, uint8_t* over,
                               uint8_t* active, uint32_t* list, uint32_t* slot_of, void* wg_counts, uint32_t* wg_offsets,
                               AdaptivePartial* partials, AdaptiveTotals* totals, int width, int rows, float threshold,
                               int window, hipStream_t stream) {
  const uint32_t npix = (uint32_t)width * (uint32_t)rows;
  const dim3 tiles((uint32_t)((width + dev::kAdTileW - 1) / dev::kAdTileW), (uint32_t)((rows + dev::kAdTileH - 1) / dev::kAdTileH));
  hipLaunchKernelGGL(dev::adaptive_classify_kernel, dim3(AdaptiveBlocks(npix)), dim3(dev::kAdBlock), 0, stream, accum,
                     moment2, counts, over, partials, npix, (double)threshold);
  hipLaunchKernelGGL(dev::adaptive_retire_kernel, tiles, dim3(dev::kAdBlock), 0, stream, over, active,
                     reinterpret_cast<uint2*>(wg_counts), width, rows, window);
  hipLaunchKernelGGL(dev::adaptive_scan_kernel, dim3(1), dim3(dev::kAdBlock), 0, stream,
                     reinterpret_cast<const uint2*>(wg_counts), wg_offsets, tiles.x * tiles.y, partials,
                     AdaptiveBlocks(npix), list, npix, totals);
  hipLaunchKernelGGL(dev::adaptive_scatter_kernel, tiles, dim3(dev::kAdBlock), 0, stream, active, wg_offsets, list,
                     slot_of, width, rows);
  return hipGetLastError();
}

}  // namespace rt2
