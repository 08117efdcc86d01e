// temporal.hip — temporal reuse of temporal.h on the GPU (rt2.h "Temporal reuse"). Kernels on
// the caller's stream, no atomics anywhere: the same input gives the same bytes every time.
//
//   history  four float4 planes of npix words each, so a tap is four 16-byte loads:
//            (ch, vh) (nrm', nh) (P', hit') (alb', mat'): denoise.hip's planes with the length in dist's place
//            and the material index in the pad's.
//   pack     one thread per pixel: colour, variance, length and the 16-float feature record into the planes.
//            The push runs it after the blend on the same stream, over the blend's result: the history is
//            replaced in place, no second packed plane is needed.
//   blend    one thread per pixel, 256 per workgroup as a 32 x 8 tile (a wave is two rows of 32 pixels).
//            The current pixel's colour, variance and length are read and replaced in place (a thread reads
//            no other pixel's), its feature record is four 16-byte loads, and the up to four taps are plain
//            global loads: a camera move maps a tile anywhere, but neighbouring threads' taps are neighbouring
//            old pixels, so a tap's loads are still mostly contiguous along a row, and each old pixel is
//            wanted by about four threads of one tile, which the L2 (and the vector L1) serve. No LDS stage.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "temporal.h"

namespace rt2 {
namespace dev {

constexpr int kTpBlock = 256;
constexpr int kTpTileW = 32, kTpTileH = 8;

// length: per-pixel floats, or null: counts (per-pixel sample counts), or null: n_scalar for every pixel.
__device__ __forceinline__ float tp_length(const float* length, const uint32_t* counts, float n_scalar, size_t i) {
  return length ? length[i] : (counts ? (float)counts[i] : n_scalar);
}

__global__ __launch_bounds__(kTpBlock) void temporal_pack_kernel(const float* __restrict__ color,
                                                                 const float* __restrict__ variance,
                                                                 const float* __restrict__ length,
                                                                 const float* __restrict__ features,
                                                                 float4* __restrict__ hist, uint32_t npix) {
  const uint32_t i = blockIdx.x * (uint32_t)kTpBlock + threadIdx.x;
  if (i >= npix) return;
  const float4* f = reinterpret_cast<const float4*>(features) + 4ull * i;
  const float4 f0 = f[0], f1 = f[1], f2 = f[2], f3 = f[3];  // slots 0-3, 4-7, 8-11, 12-15
  hist[i] = make_float4(color[3ull * i], color[3ull * i + 1], color[3ull * i + 2], variance[i]);
  hist[(size_t)npix + i] = make_float4(f1.y, f1.z, f1.w, length[i]);
  hist[2ull * npix + i] = make_float4(f0.z, f0.w, f1.x, f0.x);
  hist[3ull * npix + i] = make_float4(f2.z, f2.w, f3.x, f2.y);
}

// color / variance: read at the thread's own pixel, then written there (in place). hist null: no history.
__global__ __launch_bounds__(kTpBlock) void temporal_blend_kernel(float* color, float* variance, const float* length,
                                                                  const uint32_t* __restrict__ counts, float n_scalar,
                                                                  const float* __restrict__ features,
                                                                  const float4* __restrict__ hist, TemporalCamera cam,
                                                                  const float* __restrict__ materials, int n_materials,
                                                                  int type_bits, TemporalParams k, float* out_length,
                                                                  int width, int height) {
  const int x = (int)blockIdx.x * kTpTileW + (int)(threadIdx.x & 31u);
  const int y = (int)blockIdx.y * kTpTileH + (int)(threadIdx.x >> 5);
  if (x >= width || y >= height) return;
  const size_t npix = (size_t)width * (size_t)height;
  const size_t i = (size_t)y * (size_t)width + (size_t)x;
  const float c[3] = {color[3 * i], color[3 * i + 1], color[3 * i + 2]};
  const float v = variance[i];
  const float n = tp_length(length, counts, n_scalar, i);
  if (!hist) {  // as a history of length 0 everywhere
    out_length[i] = DenoisePixelFinite(c, v) ? n : 0.0f;
    return;
  }
  const float4* fp = reinterpret_cast<const float4*>(features) + 4 * i;
  const float4 f0 = fp[0], f1 = fp[1], f2 = fp[2], f3 = fp[3];
  const float f[16] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w, f2.x, f2.y, f2.z, f2.w, f3.x, f3.y, f3.z, f3.w};
  const auto fetch = [&](int qx, int qy) {  // inside the image (TemporalResolvePixel): j < npix
    const size_t j = (size_t)qy * (size_t)width + (size_t)qx;
    const float4 a = hist[j], b = hist[npix + j], p = hist[2 * npix + j], m = hist[3 * npix + j];
    return TemporalPixel{{a.x, a.y, a.z}, a.w, {b.x, b.y, b.z}, b.w, {p.x, p.y, p.z}, p.w, {m.x, m.y, m.z}, m.w};
  };
  const TemporalResult o =
      TemporalResolvePixel(c, v, n, f, cam, width, height, materials, n_materials, type_bits != 0, k, fetch);
  color[3 * i] = o.c[0];
  color[3 * i + 1] = o.c[1];
  color[3 * i + 2] = o.c[2];
  variance[i] = o.v;
  out_length[i] = o.len;
}

}  // namespace dev

// Bytes of the packed history of npix pixels.
size_t TemporalHistoryBytes(size_t npix) { return npix * 4 * sizeof(float4); }

// colour, variance, length (floats per pixel) and features into the history planes.
hipError_t LaunchTemporalPack(const float* color, const float* variance, const float* length, const float* features,
                              void* hist, uint32_t npix, hipStream_t stream) {
  const uint32_t blocks = (npix + (uint32_t)dev::kTpBlock - 1u) / (uint32_t)dev::kTpBlock;
  hipLaunchKernelGGL(dev::temporal_pack_kernel, dim3(blocks), dim3(dev::kTpBlock), 0, stream, color, variance, length, features,
                     static_cast<float4*>(hist), npix);
  return hipGetLastError();
}

// The blend over color (float3) and variance (float), replaced in place, and the length into out_length.
// length / counts / n_scalar: the current length (the first that is not null). hist: the packed history, or
// null. camera: the history's 21 camera words (host). materials: device, 8 floats per material, or null.
hipError_t LaunchTemporalBlend(float* color, float* variance, const float* length, const uint32_t* counts, float n_scalar,
                               const float* features, const void* hist, const float* camera, const float* materials,
                               int n_materials, bool type_bits, const TemporalParams& k, float* out_length, int width,
                               int height, hipStream_t stream) {
  const dim3 tiles((uint32_t)((width + dev::kTpTileW - 1) / dev::kTpTileW), (uint32_t)((height + dev::kTpTileH - 1) / dev::kTpTileH));
  TemporalCamera cam{};
  if (camera) cam = TemporalCameraOf(camera);
  hipLaunchKernelGGL(dev::temporal_blend_kernel, tiles, dim3(dev::kTpBlock), 0, stream, color, variance, length, counts, n_scalar,
                     features, static_cast<const float4*>(hist), cam, materials, n_materials, type_bits ? 1 : 0, k, out_length,
                     width, height);
  return hipGetLastError();
}

}  // namespace rt2
