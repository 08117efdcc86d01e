// denoise.hip — the variance-guided a-trous filter of denoise.h on the GPU (rt2.h "Feature buffers and
// denoiser"). Kernels on the caller's stream, no atomics anywhere: the same input gives the same bytes
// every time.
//
//   inputs   (tracer path) one thread per local pixel: colour = accum / (float)n and the variance of the mean
//            from noise.h NoiseOfPixel's float3 standard error, n the frame index or the pixel's own sample
//            count (adaptive sampling): the values non_converted_pixels and standard_error return.
//   pack     colour + variance and the 16-float feature record into four float4 planes, so a tap is four
//            16-byte loads: (c, v) (n, dist) (P, hit) (a, 0).
//   vbar     one thread per pixel: the pass's 3x3 variance average (DenoiseVbarTap), a pass of its own: it
//            reads the (c, v) and (P, hit) planes of nine neighbours that the L2 holds anyway and writes 4 bytes.
//   pass     one thread per pixel, 256 per workgroup as a 32 x 8 tile (a wave is two rows of 32 pixels: a
//            tap's loads are 512 contiguous bytes per row). The 25 taps are unrolled with constant (dx, dy).
//            kLds (steps 1 and 2): the tile and its halo of 2 * step pixels, all four planes, go to LDS first
//            (at step 2: 40 x 16 pixels x 64 bytes = 40 KiB, three workgroups per CU); without it, and at
//            every larger step, the taps are read from global memory, where a row's taps are still coalesced
//            along x. Which of the two the small steps take is the caller's choice (capi.cpp: the measured
//            default).
//   unpack   the last pass's (c, v) plane into float3 colour and float variance.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "denoise.h"
#include "kernels.h"
#include "noise.h"

namespace rt2 {
namespace dev {

constexpr int kDnBlock = 256;
constexpr int kDnTileW = 32, kDnTileH = 8;
constexpr int kDnLdsStepMax = 2;                  // largest step staged in LDS
constexpr int kDnHaloMax = 2 * kDnLdsStepMax;     // pixels of halo on each side at that step
constexpr int kDnLdsPixels = (kDnTileW + 2 * kDnHaloMax) * (kDnTileH + 2 * kDnHaloMax);

__global__ __launch_bounds__(kDnBlock) void denoise_inputs_kernel(const float* __restrict__ accum,
                                                                  const float* __restrict__ moment2,
                                                                  const uint32_t* __restrict__ counts,
                                                                  float* __restrict__ color, float* __restrict__ variance,
                                                                  uint32_t npix, long long n_frames) {
  const uint32_t i = blockIdx.x * (uint32_t)kDnBlock + threadIdx.x;
  if (i >= npix) return;
  const float a[3] = {accum[3ull * i], accum[3ull * i + 1], accum[3ull * i + 2]};
  const float q[3] = {moment2[3ull * i], moment2[3ull * i + 1], moment2[3ull * i + 2]};
  const int64_t n = counts ? (int64_t)counts[i] : (int64_t)n_frames;
  const float fn = (float)n;
  color[3ull * i] = a[0] / fn;
  color[3ull * i + 1] = a[1] / fn;
  color[3ull * i + 2] = a[2] / fn;
  const PixelNoise pn = NoiseOfPixel(a, q, n);
  variance[i] = DenoiseVarianceOfSem(pn.sem);
}

__global__ __launch_bounds__(kDnBlock) void denoise_pack_kernel(const float* __restrict__ color,
                                                                const float* __restrict__ variance,
                                                                const float* __restrict__ features,
                                                                float4* __restrict__ cv, float4* __restrict__ gn,
                                                                float4* __restrict__ gp, float4* __restrict__ ga,
                                                                uint32_t npix) {
  const uint32_t i = blockIdx.x * (uint32_t)kDnBlock + threadIdx.x;
  if (i >= npix) return;
  cv[i] = make_float4(color[3ull * i], color[3ull * i + 1], color[3ull * i + 2], variance[i]);
  const float4* f = reinterpret_cast<const float4*>(features) + 4ull * i;
  const float4 f0 = f[0], f1 = f[1], f2 = f[2], f3 = f[3];  // slots 0-3, 4-7, 8-11, 12-15
  gn[i] = make_float4(f1.y, f1.z, f1.w, f3.y);
  gp[i] = make_float4(f0.z, f0.w, f1.x, f0.x);
  ga[i] = make_float4(f2.z, f2.w, f3.x, 0.0f);
}

__global__ __launch_bounds__(kDnBlock) void denoise_unpack_kernel(const float4* __restrict__ cv, float* __restrict__ color,
                                                                  float* __restrict__ variance, uint32_t npix) {
  const uint32_t i = blockIdx.x * (uint32_t)kDnBlock + threadIdx.x;
  if (i >= npix) return;
  const float4 p = cv[i];
  color[3ull * i] = p.x;
  color[3ull * i + 1] = p.y;
  color[3ull * i + 2] = p.z;
  if (variance) variance[i] = p.w;
}

__global__ __launch_bounds__(kDnBlock) void denoise_vbar_kernel(const float4* __restrict__ cv, const float4* __restrict__ gp,
                                                                float* __restrict__ vbar, int width, int height) {
  const int x = (int)blockIdx.x * kDnTileW + (int)(threadIdx.x & 31u);
  const int y = (int)blockIdx.y * kDnTileH + (int)(threadIdx.x >> 5);
  if (x >= width || y >= height) return;
  const size_t i = (size_t)y * (size_t)width + (size_t)x;
  const float hit_p = gp[i].w;
  DenoiseVbarSums s{0.0f, 0.0f};
#pragma unroll
  for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
      const int qx = x + dx, qy = y + dy;
      if (qx < 0 || qx >= width || qy < 0 || qy >= height) continue;
      const size_t j = (size_t)qy * (size_t)width + (size_t)qx;
      const float4 c = cv[j];
      const float cq[3] = {c.x, c.y, c.z};
      DenoiseVbarTap(s, hit_p, cq, c.w, gp[j].w, dx, dy);
    }
  }
  // (a pixel that is not finite is skipped by its own centre tap: sw may be 0; the pass never reads its vbar)
  vbar[i] = s.sw > 0.0f ? DenoiseVbarFinish(s) : 0.0f;
}

__device__ __forceinline__ DenoisePixel dn_pixel(float4 c, float4 n, float4 p, float4 a) {
  return DenoisePixel{{c.x, c.y, c.z}, c.w, {n.x, n.y, n.z}, n.w, {p.x, p.y, p.z}, p.w, {a.x, a.y, a.z}, 0.0f};
}

template <bool kLds>
__global__ __launch_bounds__(kDnBlock) void denoise_pass_kernel(const float4* __restrict__ cv, const float* __restrict__ vbar,
                                                                const float4* __restrict__ gn, const float4* __restrict__ gp,
                                                                const float4* __restrict__ ga, float4* __restrict__ out,
                                                                int width, int height, int step, DenoiseParams k) {
  const int x0 = (int)blockIdx.x * kDnTileW, y0 = (int)blockIdx.y * kDnTileH;
  const int tx = (int)(threadIdx.x & 31u), ty = (int)(threadIdx.x >> 5);
  const int x = x0 + tx, y = y0 + ty;
  // kLds: the tile with a halo of 2 * step pixels (step <= kDnLdsStepMax, the launcher's choice), row pitch
  // kDnTileW + 4 * step; pixels outside the image are left unwritten and never read (a tap outside is skipped)
  __shared__ float4 s_cv[kLds ? kDnLdsPixels : 1], s_n[kLds ? kDnLdsPixels : 1], s_p[kLds ? kDnLdsPixels : 1],
      s_a[kLds ? kDnLdsPixels : 1];
  const int halo = 2 * step, pitch = kDnTileW + 2 * halo;
  if constexpr (kLds) {
    const int rows = kDnTileH + 2 * halo;
    for (int e = (int)threadIdx.x; e < pitch * rows; e += kDnBlock) {
      const int ry = e / pitch, rx = e - ry * pitch;
      const int gx = x0 - halo + rx, gy = y0 - halo + ry;
      if (gx >= 0 && gx < width && gy >= 0 && gy < height) {
        const size_t j = (size_t)gy * (size_t)width + (size_t)gx;
        s_cv[e] = cv[j];
        s_n[e] = gn[j];
        s_p[e] = gp[j];
        s_a[e] = ga[j];
      }
    }
    __syncthreads();
  }
  if (x >= width || y >= height) return;
  const size_t i = (size_t)y * (size_t)width + (size_t)x;
  const auto fetch = [&](int qx, int qy) {
    if constexpr (kLds) {
      const int e = (qy - y0 + halo) * pitch + (qx - x0 + halo);
      return dn_pixel(s_cv[e], s_n[e], s_p[e], s_a[e]);
    } else {
      const size_t j = (size_t)qy * (size_t)width + (size_t)qx;
      return dn_pixel(cv[j], gn[j], gp[j], ga[j]);
    }
  };
  const DenoisePixel p = fetch(x, y);
  if (!DenoisePixelFinite(p.c, p.v)) {
    out[i] = make_float4(p.c[0], p.c[1], p.c[2], p.v);
    return;
  }
  const DenoiseCentre pc = DenoiseCentreOf(p, vbar[i], k);
  DenoiseSums s = DenoiseSumsZero();
#pragma unroll
  for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = x + step * dx, qy = y + step * dy;
      if (qx < 0 || qx >= width || qy < 0 || qy >= height) continue;
      DenoiseTap(s, p, pc, (dx == 0 && dy == 0) ? p : fetch(qx, qy), dx, dy, k);
    }
  }
  float oc[3], ov;
  DenoiseFinish(s, p, oc, ov);
  out[i] = make_float4(oc[0], oc[1], oc[2], ov);
}

}  // namespace dev

namespace {
dim3 DnTiles(int width, int height) {
  return dim3((uint32_t)((width + dev::kDnTileW - 1) / dev::kDnTileW), (uint32_t)((height + dev::kDnTileH - 1) / dev::kDnTileH));
}
uint32_t DnBlocks(uint32_t npix) { return (npix + (uint32_t)dev::kDnBlock - 1u) / (uint32_t)dev::kDnBlock; }
}  // namespace

// Bytes of device scratch a denoise of npix pixels needs: float3 colour, float variance (the inputs / the
// result), two (c, v) planes, three feature planes, vbar.
size_t DenoiseScratchBytes(size_t npix) { return npix * (12 + 4 + 2 * 16 + 3 * 16 + 4); }

// The tracer path's inputs into the scratch's colour and variance planes.
hipError_t LaunchDenoiseInputs(const float* accum, const float* moment2, const uint32_t* counts, void* scratch,
                               uint32_t npix, int64_t n_frames, hipStream_t stream) {
  float* color = static_cast<float*>(scratch);
  float* variance = color + 3ull * npix;
  hipLaunchKernelGGL(dev::denoise_inputs_kernel, dim3(DnBlocks(npix)), dim3(dev::kDnBlock), 0, stream, accum, moment2, counts,
                     color, variance, npix, (long long)n_frames);
  return hipGetLastError();
}

// The filter over the scratch's colour and variance planes (device pointers scratch, scratch + 3 * npix
// floats; filled by LaunchDenoiseInputs or a copy) and `features` (device, 16 floats per pixel); the result
// replaces the colour and variance planes. lds: steps 1 and 2 stage their tile in LDS.
hipError_t LaunchDenoise(void* scratch, const float* features, int width, int height, const DenoiseParams& k, bool lds,
                         hipStream_t stream) {
  const uint32_t npix = (uint32_t)width * (uint32_t)height;
  float* color = static_cast<float*>(scratch);
  float* variance = color + 3ull * npix;
  float4* cv0 = reinterpret_cast<float4*>(variance + npix);
  float4* cv1 = cv0 + npix;
  float4* gn = cv1 + npix;
  float4* gp = gn + npix;
  float4* ga = gp + npix;
  float* vbar = reinterpret_cast<float*>(ga + npix);
  const dim3 tiles = DnTiles(width, height), block(dev::kDnBlock);
  hipLaunchKernelGGL(dev::denoise_pack_kernel, dim3(DnBlocks(npix)), block, 0, stream, color, variance, features, cv0, gn, gp,
                     ga, npix);
  float4* src = cv0;
  float4* dst = cv1;
  for (int it = 0; it < k.iterations; it++) {
    const int step = 1 << it;
    hipLaunchKernelGGL(dev::denoise_vbar_kernel, tiles, block, 0, stream, src, gp, vbar, width, height);
    if (lds && step <= dev::kDnLdsStepMax)
      hipLaunchKernelGGL(dev::denoise_pass_kernel<true>, tiles, block, 0, stream, src, vbar, gn, gp, ga, dst, width, height,
                         step, k);
    else
      hipLaunchKernelGGL(dev::denoise_pass_kernel<false>, tiles, block, 0, stream, src, vbar, gn, gp, ga, dst, width, height,
                         step, k);
    float4* t = src;
    src = dst;
    dst = t;
  }
  hipLaunchKernelGGL(dev::denoise_unpack_kernel, dim3(DnBlocks(npix)), block, 0, stream, src, color, variance, npix);
  return hipGetLastError();
}

}  // namespace rt2
