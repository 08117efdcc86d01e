// kernels.h — the host-callable functions the seven .hip files define (render, gather, noise, adaptive,
// denoise, temporal, present): kernel launchers and the small queries beside them. Included by the host side and
// by every .hip file, so the compiler checks each definition against the one declaration here.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "adaptive.h"
#include "ambient.h"
#include "denoise.h"
#include "noise.h"
#include "radiance.h"
#include "rt2_layout.h"
#include "temporal.h"

namespace rt2 {
// render.hip
hipError_t LaunchRender(const RenderParams& p, int variant, bool stats, int grid, hipStream_t stream);
int RenderBlocksPerCU(int variant, int mode, bool stats, size_t lds_bytes, bool list = false, bool flat = false);
hipError_t LaunchAccumulateList(const float* samples, const uint32_t* list, float* accum, float* moment2,
                                uint32_t* counts, uint8_t* pixels, uint32_t nslots, int n_frames, hipStream_t stream);
hipError_t LaunchAccumulate(const float* samples, float* accum, float* moment2, uint8_t* pixels, uint32_t npix,
                            int n_frames, int frame_idx, hipStream_t stream);
hipError_t LaunchSelftest(int which, unsigned long long n, uint32_t seed, unsigned long long* d_out, hipStream_t stream);
hipError_t LaunchFeatures(const RenderParams& p, float* out, hipStream_t stream);
hipError_t LaunchQuery(const RenderParams& p, int variant, const float* rays, float* out, uint32_t n, hipStream_t stream);
hipError_t LaunchOcclusion(const RenderParams& p, int variant, const float* rays, int8_t* out, uint32_t n,
                           hipStream_t stream);
hipError_t LaunchAmbient(const RenderParams& p, int variant, const AmbientSource& src, uint32_t n_points, uint32_t s0,
                         uint32_t k, Magic k_div, uint32_t* counts, hipStream_t stream);
hipError_t LaunchRadiance(const RenderParams& p, int variant, const float* rays, const uint32_t* streams, uint32_t index0,
                          uint32_t n, uint32_t s0, uint32_t k, Magic k_div, const RadianceArgs& a, uint32_t wave_items,
                          uint32_t grid, float* slots, float* out_sum, uint32_t* out_rays, hipStream_t stream);
size_t QueryLdsBytes(const RenderParams& p);
int RenderMode(const RenderParams& p);
int RenderBlockSize();
int RenderVariant(uint32_t features);
uint32_t RenderVariantFeatures(int v);
size_t RenderLdsBytes(const RenderParams& p);
bool RenderTakesHitTable(int variant, int mode, bool stats);
bool RenderTakesFlat(int variant, int mode, bool stats, bool list);
// gather.hip
hipError_t LaunchDeinterleave(const float* stacks, float* image, float* image_nc, uint8_t* pixels, int width, int height, int band_h,
                              int world, int max_rows, int frame_idx, hipStream_t stream);
hipError_t LaunchDeinterleaveEstimate(const float* stacks, const float* stacks2, float* image, float* image_nc,
                                      uint8_t* pixels, float* variance, int width, int height, int band_h, int world,
                                      int max_rows, int frame_idx, hipStream_t stream);
hipError_t LaunchDeinterleaveAdaptive(const float* stacks, const float* stacks2, const uint32_t* counts, float* image,
                                      float* image_nc, uint8_t* pixels, float* variance, uint32_t* image_counts, int width,
                                      int height, int band_h, int world, int max_rows, hipStream_t stream);
// noise.hip
uint32_t NoiseBlocks(uint32_t npix);
hipError_t LaunchNoise(const float* accum, const float* moment2, const uint32_t* counts, float* sem,
                       NoisePartial* partials, uint32_t npix, int64_t n_frames, float threshold, hipStream_t stream);
// adaptive.hip
uint32_t AdaptiveBlocks(uint32_t npix);
uint32_t AdaptiveTiles(int width, int rows);
hipError_t LaunchAdaptiveCheck(const float* accum, const float* moment2, const uint32_t* counts, uint8_t* over,
                               uint8_t* active, uint32_t* list, uint32_t* slot_of, void* wg_counts, uint32_t* wg_offsets,
                               AdaptivePartial* partials, AdaptiveTotals* totals, int width, int rows, float threshold,
                               int window, hipStream_t stream);
// denoise.hip
size_t DenoiseScratchBytes(size_t npix);
hipError_t LaunchDenoiseInputs(const float* accum, const float* moment2, const uint32_t* counts, void* scratch,
                               uint32_t npix, int64_t n_frames, hipStream_t stream);
hipError_t LaunchDenoise(void* scratch, const float* features, int width, int height, const DenoiseParams& k, bool lds,
                         hipStream_t stream);
// temporal.hip
size_t TemporalHistoryBytes(size_t npix);
hipError_t LaunchTemporalPack(const float* color, const float* variance, const float* length, const float* features,
                              void* hist, uint32_t npix, hipStream_t stream);
hipError_t LaunchTemporalBlend(float* color, float* variance, const float* length, const uint32_t* counts, float n_scalar,
                               const float* features, const void* hist, const float* camera, const float* materials,
                               int n_materials, bool type_bits, const TemporalParams& k, float* out_length, int width,
                               int height, hipStream_t stream);
// present.hip
hipError_t LaunchPresent(const float* color, void* rgba, uint32_t npix, hipStream_t stream);
}  // namespace rt2
