// capi_estimate.cpp — the noise estimate and adaptive sampling entry points of include/rt2.h (over noise.hip and
// adaptive.hip).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "tracer.h"

using namespace rt2;
using namespace rt2::detail;

namespace {
float NoiseRms(const rt2_noise& o) {
  const uint64_t finite = o.pixels - o.nonfinite;
  return finite ? (float)std::sqrt(o.sum_sq / (double)finite) : 0.0f;
}

// The noise kernel over a one-GPU tracer's local pixels: the float3 standard error into sem_host
// (or null) and the scalars into out (or null). The partials are added up in block order.
int NoiseLocal(rt2_tracer* t, float threshold, float* sem_host, rt2_noise* out) {
  if (!t->moments_on) return Fail(RT2_ERR_INVALID, "moments not enabled (rt2_tracer_enable_moments)");
  int rc = Sync(t);
  if (rc != RT2_OK) return rc;
  if (t->frame_idx < 2) return Fail(RT2_ERR_INVALID, "the noise estimate needs at least 2 frames");
  const size_t n = (size_t)t->width * (size_t)t->local_rows;
  rt2_noise o;
  memset(&o, 0, sizeof(o));
  o.frames = t->frame_idx;
  o.pixels = n;
  if (n) {
    HIP_TRY(hipSetDevice(t->device));
    const size_t blocks = NoiseBlocks((uint32_t)n);
    if (blocks * sizeof(NoisePartial) > t->d_noise.bytes()) {
      HIP_TRY(t->d_noise.Grow(blocks * sizeof(NoisePartial)));
      NoteDeviceBytes(t);
    }
    DeviceBuffer d_sem;
    if (sem_host) HIP_TRY(d_sem.Alloc(n * 3 * sizeof(float)));
    std::vector<NoisePartial> parts(blocks);
    // (adaptive sampling: each pixel's estimate rests on its own sample count)
    hipError_t e = LaunchNoise(t->d_accum.get<float>(), t->d_moment2.get<float>(),
                               t->adaptive_on ? t->d_counts.get<uint32_t>() : nullptr, d_sem.get<float>(),
                               t->d_noise.get<NoisePartial>(), (uint32_t)n, t->frame_idx, threshold, t->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(parts.data(), t->d_noise.get<NoisePartial>(), blocks * sizeof(NoisePartial), hipMemcpyDeviceToHost,
                         t->stream);
    if (e == hipSuccess && sem_host)
      e = hipMemcpyAsync(sem_host, d_sem.get<float>(), n * 3 * sizeof(float), hipMemcpyDeviceToHost, t->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    t->host_waits++;
    if (e != hipSuccess) return HipFail(e, "noise estimate");
    double mx = 0.0;
    for (const NoisePartial& p : parts) {
      o.sum_sq = o.sum_sq + p.sum_sq;
      mx = p.max_err > mx ? p.max_err : mx;
      o.below += p.below;
      o.nonfinite += p.nonfinite;
    }
    o.max_err = (float)mx;
  }
  o.rms = NoiseRms(o);
  if (out) *out = o;
  return RT2_OK;
}
}  // namespace

extern "C" {

// ---- noise estimate (rt2.h "Noise estimate and render-until-converged") ----
int rt2_tracer_enable_moments(rt2_tracer* t, int on) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  RT2_FORWARD(t, rt2_tracer_enable_moments(p, on));
  if (!on && t->adaptive_on) return Fail(RT2_ERR_INVALID, "enable_moments(0): adaptive sampling is on and needs the moments");
  int rc = Sync(t);
  if (rc != RT2_OK) return rc;
  t->moments_on = on != 0;
  if ((rc = Realloc(t)) != RT2_OK) return rc;
  return ResetFrame(t);
}

int rt2_tracer_moments(rt2_tracer* t, float* out) {
  if (!t || !out) return Fail(RT2_ERR_INVALID, "null argument");
  if (IsMulti(t))
    return PlacePartRows(t, out, 3, [](rt2_tracer* p, float* rows) { return rt2_tracer_moments(p, rows); });
  if (!t->moments_on) return Fail(RT2_ERR_INVALID, "moments not enabled (rt2_tracer_enable_moments)");
  int rc = Sync(t);
  if (rc != RT2_OK) return rc;
  size_t n = (size_t)t->width * (size_t)t->local_rows;
  if (n) HIP_TRY(hipMemcpy(out, t->d_moment2.get<float>(), n * 3 * sizeof(float), hipMemcpyDeviceToHost));
  return RT2_OK;
}

int rt2_tracer_standard_error(rt2_tracer* t, float* out) {
  if (!t || !out) return Fail(RT2_ERR_INVALID, "null argument");
  if (IsMulti(t))
    return PlacePartRows(t, out, 3, [](rt2_tracer* p, float* rows) { return rt2_tracer_standard_error(p, rows); });
  return NoiseLocal(t, 0.0f, out, nullptr);
}

int rt2_tracer_noise(rt2_tracer* t, float threshold, rt2_noise* out) {
  if (!t || !out) return Fail(RT2_ERR_INVALID, "null argument");
  if (!IsMulti(t)) return NoiseLocal(t, threshold, nullptr, out);
  rt2_noise sum;
  memset(&sum, 0, sizeof(sum));
  for (rt2_tracer* p : t->parts) {
    rt2_noise o;
    int rc = NoiseLocal(p, threshold, nullptr, &o);
    if (rc != RT2_OK) return rc;
    sum.frames = o.frames;
    sum.pixels += o.pixels;
    sum.below += o.below;
    sum.nonfinite += o.nonfinite;
    sum.sum_sq = sum.sum_sq + o.sum_sq;
    sum.max_err = std::max(sum.max_err, o.max_err);
  }
  sum.rms = NoiseRms(sum);
  *out = sum;
  return RT2_OK;
}

int rt2_tracer_render_until(rt2_tracer* t, float target_rms, int min_frames, int max_frames, int check_every,
                            rt2_noise* out) {
  if (!t || !out) return Fail(RT2_ERR_INVALID, "null argument");
  if (!(target_rms >= 0.0f) || min_frames < 0 || max_frames < 0 || check_every < 0)
    return Fail(RT2_ERR_INVALID, "render_until: need target_rms >= 0, min_frames, max_frames, check_every >= 0");
  rt2_tracer* first = IsMulti(t) ? t->parts[0] : t;
  if (!first->moments_on) return Fail(RT2_ERR_INVALID, "moments not enabled (rt2_tracer_enable_moments)");
  int step = check_every;
  if (step == 0) {  // one sweep of the sqrt_spp x sqrt_spp strata (RayTracer.cpp:59-60)
    const int sq = first->camera.Params().sqrt_spp;
    if (sq <= 0) return Fail(RT2_ERR_INVALID, "samples_per_pixel gives sqrt_spp = 0");
    step = (int)std::min<int64_t>((int64_t)sq * sq, 0x7FFFFFFF);
  }
  const int64_t first_check = std::max(min_frames, 2);
  memset(out, 0, sizeof(*out));
  int64_t f = rt2_tracer_frame_idx(t);
  while (f < max_frames) {
    int rc = rt2_tracer_render(t, (int)std::min<int64_t>(step, max_frames - f));
    if (rc != RT2_OK) return rc;
    f = rt2_tracer_frame_idx(t);
    if (f < first_check) continue;
    if ((rc = rt2_tracer_noise(t, target_rms, out)) != RT2_OK) return rc;
    if (out->rms <= target_rms && out->nonfinite == 0) return RT2_OK;
  }
  // no step ended in a check (max_frames reached before, or below min_frames): the image as it stands
  if (out->frames != f && f >= 2) return rt2_tracer_noise(t, target_rms, out);
  return RT2_OK;
}
}  // extern "C"

// ---- adaptive sampling (rt2.h "Adaptive sampling") ----
int rt2::detail::EnqueueAdaptiveCheck(rt2_tracer* t, float threshold, int window, AdaptiveTotals* host,
                                      AdaptiveTotals** d_totals) {
  const size_t n = (size_t)t->width * (size_t)t->local_rows;
  if (host) memset(host, 0, sizeof(*host));
  if (d_totals) *d_totals = nullptr;
  if (n == 0) return RT2_OK;
  HIP_TRY(hipSetDevice(t->device));
  // the check's scratch: [tiles] uint2 counts, [tiles] offsets, then (8-byte aligned) partials and totals
  const size_t tiles = AdaptiveTiles(t->width, t->local_rows), blocks = AdaptiveBlocks((uint32_t)n);
  char* base = t->d_ad_scratch.get<char>();
  uint32_t* offsets = reinterpret_cast<uint32_t*>(base + tiles * 8);
  const size_t part_at = (tiles * 12 + 7) / 8 * 8;
  AdaptivePartial* partials = reinterpret_cast<AdaptivePartial*>(base + part_at);
  AdaptiveTotals* totals = reinterpret_cast<AdaptiveTotals*>(base + part_at + blocks * sizeof(AdaptivePartial));
  if (part_at + blocks * sizeof(AdaptivePartial) + sizeof(AdaptiveTotals) > t->d_ad_scratch.bytes())
    return Fail(RT2_ERR_INVALID, "adaptive_check: scratch buffer too small");
  hipError_t e = LaunchAdaptiveCheck(t->d_accum.get<float>(), t->d_moment2.get<float>(), t->d_counts.get<uint32_t>(),
                                     t->d_over.get<uint8_t>(), t->d_active.get<uint8_t>(), t->d_list.get<uint32_t>(),
                                     t->d_slot_of.get<uint32_t>(), base, offsets, partials, totals, t->width,
                                     t->local_rows, threshold, window, t->stream);
  if (e == hipSuccess && host) e = hipMemcpyAsync(host, totals, sizeof(*host), hipMemcpyDeviceToHost, t->stream);
  if (e != hipSuccess) return HipFail(e, "adaptive check");
  if (d_totals) *d_totals = totals;
  return RT2_OK;
}

int rt2::detail::FinishAdaptiveCheck(rt2_tracer* t, const AdaptiveTotals& h, rt2_adaptive* out) {
  const size_t n = (size_t)t->width * (size_t)t->local_rows;
  rt2_adaptive o;
  memset(&o, 0, sizeof(o));
  o.frames = t->frame_idx;
  o.pixels = n;
  if (n) {
    if (h.active > n) return Fail(RT2_ERR_HIP, "adaptive check: active count out of range");
    t->n_active = (uint32_t)h.active;
    o.active = h.active;
    o.retired = h.retired;
    o.samples = h.samples;
    o.nonfinite = h.nonfinite;
  }
  t->last_check = o;
  if (out) *out = o;
  return RT2_OK;
}

int rt2::detail::SampleCountsLocal(rt2_tracer* t, uint32_t* out) {
  int rc = Sync(t);
  if (rc != RT2_OK) return rc;
  size_t n = (size_t)t->width * (size_t)t->local_rows;
  if (n) HIP_TRY(hipMemcpy(out, t->d_counts.get<uint32_t>(), n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RT2_OK;
}

namespace {
constexpr const char* kAdaptiveOffMsg = "adaptive sampling not enabled (rt2_tracer_enable_adaptive)";
constexpr const char* kImageAdaptiveOffMsg =
    "adaptive sampling of the gathered image not enabled (rt2_tracer_image_enable_adaptive)";

// What enable_adaptive needs of a one-GPU tracer to switch it on, under the call's name.
int AdaptiveNeeds(const rt2_tracer* t, const char* call) {
  if (!t->moments_on)
    return Fail(RT2_ERR_INVALID, std::string(call) + ": moments not enabled (rt2_tracer_enable_moments)");
  // the kernels over an active list exist for the threaded traversal, the default mode: refused here, not
  // at the first launch after a pixel has retired
  if (!t->use_linear || !t->lin_len)
    return Fail(RT2_ERR_INVALID, std::string(call) + ": needs the threaded traversal (the scene has none, or RT2_NO_LINEAR)");
  return RT2_OK;
}

// Switches adaptive sampling on a one-GPU tracer: synchronises, reallocates (which drops the gathered image and a
// held history) and resets. image: the counts travel with the gather from now on.
int SetAdaptive(rt2_tracer* t, bool on, bool image) {
  int rc = Sync(t);
  if (rc != RT2_OK) return rc;
  t->adaptive_on = on;
  t->image_adaptive = on && image;
  if ((rc = Realloc(t)) != RT2_OK) return rc;
  return ResetFrame(t);
}

int CheckArguments(const char* call, float threshold, int window) {
  if (!(threshold >= 0.0f)) return Fail(RT2_ERR_INVALID, std::string(call) + ": threshold must be >= 0");
  if (window < 0 || window > kAdaptiveWindowMax) return Fail(RT2_ERR_INVALID, std::string(call) + ": need 0 <= window <= 64");
  return RT2_OK;
}

// The frames of one step of render_adaptive / image_render_adaptive (check_every 0: one sweep of the sqrt_spp x
// sqrt_spp strata, RayTracer.cpp:59-60).
int AdaptiveStep(rt2_tracer* first, int check_every, int* step) {
  *step = check_every;
  if (check_every == 0) {
    const int sq = first->camera.Params().sqrt_spp;
    if (sq <= 0) return Fail(RT2_ERR_INVALID, "samples_per_pixel gives sqrt_spp = 0");
    *step = (int)std::min<int64_t>((int64_t)sq * sq, 0x7FFFFFFF);
  }
  return RT2_OK;
}

// The image check's pinned host words (h_check): a joined tracer's are kCheckWords (its local totals and pixel
// count, then the sums over the ranks) with the pixel count it uploads behind them.
constexpr size_t kCheckWords = 10;
int EnsureCheckWords(rt2_tracer* t) {
  if (t->h_check) return RT2_OK;
  HIP_TRY(hipSetDevice(t->device));
  HIP_TRY(hipHostMalloc((void**)&t->h_check, (kCheckWords + 1) * sizeof(unsigned long long), hipHostMallocDefault));
  return RT2_OK;
}

void AddCheck(rt2_adaptive* sum, const rt2_adaptive& o) {
  sum->frames = o.frames;
  sum->pixels += o.pixels;
  sum->active += o.active;
  sum->retired += o.retired;
  sum->samples += o.samples;
  sum->nonfinite += o.nonfinite;
}

// The check of a joined tracer, collective: after the local check its four totals and its pixel count are copied
// beside themselves on the device and the copy is summed in place over the ranks on the tracer's stream; one host
// copy then brings both, the local totals for this rank's n_active and the whole image's for *out.
int JoinedCheck(rt2_tracer* t, float threshold, int window, rt2_adaptive* out) {
  static_assert(sizeof(AdaptiveTotals) == 4 * sizeof(unsigned long long), "the all-reduce sums four words and the pixels");
  int rc = EnsureCheckWords(t);
  if (rc != RT2_OK) return rc;
  HIP_TRY(hipSetDevice(t->device));
  if (!t->d_check_sum) {
    HIP_TRY(t->d_check_sum.Alloc(kCheckWords * sizeof(unsigned long long)));
    NoteDeviceBytes(t);
  }
  unsigned long long* d = t->d_check_sum.get<unsigned long long>();
  unsigned long long* h = t->h_check;
  AdaptiveTotals* d_totals = nullptr;
  if ((rc = EnqueueAdaptiveCheck(t, threshold, window, nullptr, &d_totals)) != RT2_OK) return rc;
  h[kCheckWords] = (unsigned long long)t->width * (unsigned long long)t->local_rows;
  if (d_totals)
    HIP_TRY(hipMemcpyAsync(d, d_totals, sizeof(AdaptiveTotals), hipMemcpyDeviceToDevice, t->stream));
  else  // a rank without a pixel adds nothing
    HIP_TRY(hipMemsetAsync(d, 0, sizeof(AdaptiveTotals), t->stream));
  HIP_TRY(hipMemcpyAsync(d + 4, h + kCheckWords, sizeof(unsigned long long), hipMemcpyHostToDevice, t->stream));
  HIP_TRY(hipMemcpyAsync(d + 5, d, 5 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, t->stream));
  NCCL_TRY(ncclAllReduce(d + 5, d + 5, 5, ncclUint64, ncclSum, t->comm, t->stream));
  hipError_t e = hipMemcpyAsync(h, d, kCheckWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, t->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
  t->host_waits++;
  if (e != hipSuccess) return HipFail(e, "adaptive check");
  AdaptiveTotals local;
  memcpy(&local, h, sizeof(local));
  if ((rc = FinishAdaptiveCheck(t, local, nullptr)) != RT2_OK) return rc;
  AdaptiveTotals all;
  memcpy(&all, h + 5, sizeof(all));
  memset(out, 0, sizeof(*out));
  out->frames = t->frame_idx;
  out->pixels = h[9];
  out->active = all.active;
  out->retired = all.retired;
  out->samples = all.samples;
  out->nonfinite = all.nonfinite;
  return RT2_OK;
}

// rt2_tracer_image_adaptive_check after its argument checks.
int ImageCheck(rt2_tracer* t, float threshold, int window, rt2_adaptive* out) {
  rt2_tracer* first = IsMulti(t) ? t->parts[0] : t;
  if (!first->image_adaptive) return Fail(RT2_ERR_INVALID, kImageAdaptiveOffMsg);
  if (first->frame_idx + first->queued < 2) return Fail(RT2_ERR_INVALID, "image_adaptive_check needs at least 2 frames");
  std::vector<rt2_tracer*> one{t};
  const std::vector<rt2_tracer*>& ranks = IsMulti(t) ? t->parts : one;
  int rc;
  for (rt2_tracer* p : ranks)
    if ((rc = Flush(p)) != RT2_OK) return rc;
  if (!IsMulti(t) && t->comm) return JoinedCheck(t, threshold, window, out);
  // every part's check and the copy of its totals are enqueued before any of them is waited for: the checks of a
  // create_multi tracer overlap across the GPUs, and the host waits once per part
  for (rt2_tracer* p : ranks) {
    if ((rc = EnsureCheckWords(p)) != RT2_OK) return rc;
    if ((rc = EnqueueAdaptiveCheck(p, threshold, window, reinterpret_cast<AdaptiveTotals*>(p->h_check), nullptr)) != RT2_OK)
      return rc;
  }
  rt2_adaptive sum;
  memset(&sum, 0, sizeof(sum));
  for (rt2_tracer* p : ranks) {
    HIP_TRY(hipSetDevice(p->device));
    const hipError_t e = hipStreamSynchronize(p->stream);
    p->host_waits++;
    if (e != hipSuccess) return HipFail(e, "adaptive check");
    AdaptiveTotals h;
    memcpy(&h, p->h_check, sizeof(h));
    rt2_adaptive o;
    if ((rc = FinishAdaptiveCheck(p, h, &o)) != RT2_OK) return rc;
    AddCheck(&sum, o);
  }
  *out = sum;
  return RT2_OK;
}
}  // namespace

extern "C" {

int rt2_tracer_enable_adaptive(rt2_tracer* t, int on) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  if (IsMulti(t) || t->comm)
    return Fail(RT2_ERR_INVALID, "enable_adaptive: not on a multi-GPU or joined tracer (their gathered image divides by "
                                 "one frame index); a set_partition tracer works");
  int rc = on ? AdaptiveNeeds(t, "enable_adaptive") : RT2_OK;
  if (rc != RT2_OK) return rc;
  return SetAdaptive(t, on != 0, false);
}

int rt2_tracer_sample_counts(rt2_tracer* t, uint32_t* out) {
  if (!t || !out) return Fail(RT2_ERR_INVALID, "null argument");
  if (IsMulti(t) || t->comm || !t->adaptive_on) return Fail(RT2_ERR_INVALID, kAdaptiveOffMsg);
  return SampleCountsLocal(t, out);
}

int rt2_tracer_adaptive_check(rt2_tracer* t, float threshold, int window, rt2_adaptive* out) {
  if (!t || !out) return Fail(RT2_ERR_INVALID, "null argument");
  if (IsMulti(t) || t->comm || !t->adaptive_on) return Fail(RT2_ERR_INVALID, kAdaptiveOffMsg);
  int rc = CheckArguments("adaptive_check", threshold, window);
  if (rc != RT2_OK) return rc;
  if ((rc = Sync(t)) != RT2_OK) return rc;
  if (t->frame_idx < 2) return Fail(RT2_ERR_INVALID, "adaptive_check needs at least 2 frames");
  AdaptiveTotals h;
  AdaptiveTotals* d_totals = nullptr;
  if ((rc = EnqueueAdaptiveCheck(t, threshold, window, &h, &d_totals)) != RT2_OK) return rc;
  if (d_totals) {
    const hipError_t e = hipStreamSynchronize(t->stream);
    t->host_waits++;
    if (e != hipSuccess) return HipFail(e, "adaptive check");
  }
  return FinishAdaptiveCheck(t, h, out);
}

int rt2_tracer_render_adaptive(rt2_tracer* t, float threshold, int window, int min_frames, int max_frames,
                               int check_every, rt2_adaptive* out) {
  if (!t || !out) return Fail(RT2_ERR_INVALID, "null argument");
  if (IsMulti(t) || t->comm || !t->adaptive_on) return Fail(RT2_ERR_INVALID, kAdaptiveOffMsg);
  if (!(threshold >= 0.0f) || window < 0 || window > kAdaptiveWindowMax || min_frames < 0 || max_frames < 0 ||
      check_every < 0)
    return Fail(RT2_ERR_INVALID, "render_adaptive: need threshold >= 0, 0 <= window <= 64, min_frames, max_frames, "
                                 "check_every >= 0");
  int step;
  int rc = AdaptiveStep(t, check_every, &step);
  if (rc != RT2_OK) return rc;
  const int64_t first_check = std::max(min_frames, 2);
  memset(out, 0, sizeof(*out));
  int64_t f = rt2_tracer_frame_idx(t);
  while (f < max_frames) {
    rc = rt2_tracer_render(t, (int)std::min<int64_t>(step, max_frames - f));
    if (rc != RT2_OK) return rc;
    f = rt2_tracer_frame_idx(t);
    if (f < first_check) continue;
    if ((rc = rt2_tracer_adaptive_check(t, threshold, window, out)) != RT2_OK) return rc;
    if (out->active == 0) return RT2_OK;
  }
  return RT2_OK;
}

// ---- adaptive sampling of the gathered image (rt2.h) ----
int rt2_tracer_image_enable_adaptive(rt2_tracer* t, int on) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  if (!IsMulti(t) && !t->comm && t->world > 1)
    return Fail(RT2_ERR_INVALID, "image_enable_adaptive: a partitioned tracer must be joined to a communicator");
  std::vector<rt2_tracer*> one{t};
  const std::vector<rt2_tracer*>& ranks = IsMulti(t) ? t->parts : one;
  int rc;
  if (on)  // every part is asked before any of them changes
    for (const rt2_tracer* p : ranks)
      if ((rc = AdaptiveNeeds(p, "image_enable_adaptive")) != RT2_OK) return rc;
  for (rt2_tracer* p : ranks)
    if ((rc = SetAdaptive(p, on != 0, true)) != RT2_OK) return rc;
  return RT2_OK;
}

int rt2_tracer_image_adaptive_check(rt2_tracer* t, float threshold, int window, rt2_adaptive* out) {
  if (!t || !out) return Fail(RT2_ERR_INVALID, "null argument");
  int rc = CheckArguments("image_adaptive_check", threshold, window);
  if (rc != RT2_OK) return rc;
  return ImageCheck(t, threshold, window, out);
}

int rt2_tracer_image_render_adaptive(rt2_tracer* t, float threshold, int window, int min_frames, int max_frames,
                                     int check_every, rt2_adaptive* out) {
  if (!t || !out) return Fail(RT2_ERR_INVALID, "null argument");
  rt2_tracer* first = IsMulti(t) ? t->parts[0] : t;
  if (!first->image_adaptive) return Fail(RT2_ERR_INVALID, kImageAdaptiveOffMsg);
  if (!(threshold >= 0.0f) || window < 0 || window > kAdaptiveWindowMax || min_frames < 0 || max_frames < 0 ||
      check_every < 0)
    return Fail(RT2_ERR_INVALID, "image_render_adaptive: need threshold >= 0, 0 <= window <= 64, min_frames, "
                                 "max_frames, check_every >= 0");
  int step;
  int rc = AdaptiveStep(first, check_every, &step);
  if (rc != RT2_OK) return rc;
  const int64_t first_check = std::max(min_frames, 2);
  memset(out, 0, sizeof(*out));
  int64_t f = rt2_tracer_frame_idx(t);
  // (joined tracers: every rank sees the same scalars, so all of them leave the loop at the same step)
  while (f < max_frames) {
    rc = rt2_tracer_render(t, (int)std::min<int64_t>(step, max_frames - f));
    if (rc != RT2_OK) return rc;
    f = rt2_tracer_frame_idx(t);
    if (f < first_check) continue;
    if ((rc = ImageCheck(t, threshold, window, out)) != RT2_OK) return rc;
    if (out->active == 0) return RT2_OK;
  }
  return RT2_OK;
}

int rt2_tracer_image_part_adaptive(rt2_tracer* t, int part, rt2_adaptive* out) {
  if (!t || !out) return Fail(RT2_ERR_INVALID, "null argument");
  const int n = IsMulti(t) ? (int)t->parts.size() : 1;
  if (part < 0 || part >= n) return Fail(RT2_ERR_INVALID, "image_part_adaptive: part out of range");
  const rt2_tracer* p = IsMulti(t) ? t->parts[(size_t)part] : t;
  if (!p->image_adaptive) return Fail(RT2_ERR_INVALID, kImageAdaptiveOffMsg);
  if (p->last_check.frames == 0) return Fail(RT2_ERR_INVALID, "image_part_adaptive: no check since the last reset");
  *out = p->last_check;
  return RT2_OK;
}
}  // extern "C"

