// capi_query.cpp — the ray queries of include/rt2.h ("Ray queries"): the scene's closest Hit for rays the caller
// owns, over render.hip's query kernel, and whether anything is in their way, over its occlusion kernel. Planned by launch_plan.h PlanQuery; the layouts and the validity rule are
// query.h's. And "Ambient occlusion": blocked-sample counts per pixel or caller point over render.hip's ambient
// kernel, through the same buffers and chunks; planned by PlanAmbient, the rule is ambient.h's. And "Radiance
// queries": RayColorForward along the caller's rays over render.hip's radiance kernels, through the same buffers and
// chunks and a slot buffer; planned by PlanRadiance, the rule is radiance.h's.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "ambient.h"
#include "kernels.h"
#include "launch_plan.h"
#include "query.h"
#include "radiance.h"
#include "tracer.h"

using namespace rt2;
using namespace rt2::detail;

namespace {

constexpr int64_t kQueryChunkDefault = (int64_t)1 << 22;

// Most rays per launch of the host entry: RT2_QUERY_CHUNK, read at every call, rounded up to whole waves.
int64_t QueryChunk() {
  int64_t c = kQueryChunkDefault;
  if (const char* e = getenv("RT2_QUERY_CHUNK")) {
    const long long v = atoll(e);
    if (v > 0) c = std::min<long long>(v, 0x7FFFFFC0ll);
  }
  return (c + 63) / 64 * 64;
}

int CheckCall(const rt2_tracer* t, int64_t n, const void* rays, const void* out, const char* call) {
  // (the arguments first: these refusals need no tracer, so they can be checked without a device)
  if (n < 0 || n >= ((int64_t)1 << 31)) return Fail(RT2_ERR_INVALID, std::string(call) + ": need 0 <= n < 2^31");
  if (!rays || !out) return Fail(RT2_ERR_INVALID, std::string(call) + ": null pointer");
  if (!t) return Fail(RT2_ERR_INVALID, std::string(call) + ": null tracer");
  if (IsMulti(t)) return Fail(RT2_ERR_INVALID, std::string(call) + ": not on a create_multi tracer");
  return RT2_OK;
}

// The launch parameters of a query with this seed and its plan for n rays; refuses a scene no traversal serves.
int QueryParams(const rt2_tracer* t, uint64_t seed, uint32_t n, const char* call, RenderParams* p, QueryPlan* q) {
  const CameraParams no_camera = {};  // (no camera is involved)
  BaseParams(t, no_camera, p);
  p->seed_lo = (uint32_t)seed;
  p->seed_hi = (uint32_t)(seed >> 32);
  for (uint32_t r = 0; r < 10; r++) {
    p->philox_keys[2 * r] = p->seed_lo + r * 0x9E3779B9u;
    p->philox_keys[2 * r + 1] = p->seed_hi + r * 0xBB67AE85u;
  }
  p->lin = t->d_lin.get<void>();
  p->lin_wide = t->d_lin_wide.get<void>();
  p->lind = t->d_lind.get<void>();
  p->lin_len = t->use_linear ? t->lin_len : 0u;
  p->flat_xforms = t->flat_xforms ? 1u : 0u;
  const int variant = RenderVariant(t->features);  // (no kFeatDefocus: no camera is involved)
  *q = PlanQuery(p->lin_len, variant, RenderVariantFeatures(variant), p->stack_depth, n, RenderBlockSize());
  if (!q->ok)
    return Fail(RT2_ERR_INVALID, std::string(call) + ": the scene needs a traversal stack of " + std::to_string(t->max_stack) +
                                     " entries (kernel has " + std::to_string(kTraversalStack) +
                                     "): only the threaded traversal can serve it");
  return RT2_OK;
}

// The two kinds of query: what one writes per ray and the launcher of its kernel.
struct QueryKind {
  size_t out_bytes;  // per ray
  hipError_t (*launch)(const RenderParams& p, int variant, const float* rays, void* out, uint32_t n, hipStream_t stream);
};
const QueryKind kClosestHit = {kQueryHitFloats * sizeof(float),
                               [](const RenderParams& p, int variant, const float* rays, void* out, uint32_t n,
                                  hipStream_t stream) {
                                 return LaunchQuery(p, variant, rays, static_cast<float*>(out), n, stream);
                               }};
// (one byte per ray instead of a record)
const QueryKind kOcclusion = {sizeof(int8_t), [](const RenderParams& p, int variant, const float* rays, void* out,
                                                 uint32_t n, hipStream_t stream) {
                                return LaunchOcclusion(p, variant, rays, static_cast<int8_t*>(out), n, stream);
                              }};

// The host entry of either kind: queued frames first, then chunks through the tracer's two device buffers (sized for
// the closest hit's records, which hold an occlusion chunk's bytes 64 times over), one event pair per chunk, one wait.
int HostQuery(rt2_tracer* t, int64_t n, const float* rays, uint64_t seed, void* out, const QueryKind& kind,
              const char* call) {
  int rc = CheckCall(t, n, rays, out, call);
  if (rc != RT2_OK) return rc;
  if (n == 0) return RT2_OK;
  const int64_t chunk = std::min(QueryChunk(), (n + 63) / 64 * 64);
  RenderParams p;
  QueryPlan q;
  if ((rc = QueryParams(t, seed, (uint32_t)std::min(chunk, n), call, &p, &q)) != RT2_OK) return rc;
  if ((rc = Flush(t)) != RT2_OK) return rc;  // queued frames first, as a readback does
  HIP_TRY(hipSetDevice(t->device));
  const size_t ray_bytes = (size_t)chunk * kQueryRayFloats * sizeof(float);
  const size_t hit_bytes = (size_t)chunk * kQueryHitFloats * sizeof(float);
  if (ray_bytes > t->d_query_rays.bytes() || hit_bytes > t->d_query_hits.bytes()) {
    // (hipFree waits for the device: nothing queued still reads the old buffers)
    HIP_TRY(t->d_query_rays.Grow(ray_bytes));
    HIP_TRY(t->d_query_hits.Grow(hit_bytes));
    NoteDeviceBytes(t);
  }
  // one event pair per chunk around its kernel, from the tracer's pool and back to it on every way out
  std::vector<hipEvent_t> ev;
  struct Return {
    rt2_tracer* t;
    std::vector<hipEvent_t>& ev;
    ~Return() {
      for (hipEvent_t e : ev) t->event_pool.push_back(e);
    }
  } give_back{t, ev};
  hipError_t e = hipSuccess;
  for (int64_t at = 0; at < n && e == hipSuccess; at += chunk) {
    const uint32_t m = (uint32_t)std::min(chunk, n - at);
    hipEvent_t e0 = TakeEvent(t), e1 = TakeEvent(t);
    if (e0) ev.push_back(e0);
    if (e1) ev.push_back(e1);
    if (!e0 || !e1) return Fail(RT2_ERR_HIP, "event create failed");
    e = hipMemcpyAsync(t->d_query_rays.get<float>(), rays + (size_t)at * kQueryRayFloats,
                       (size_t)m * kQueryRayFloats * sizeof(float), hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess) e = hipEventRecord(e0, t->stream);
    if (e == hipSuccess) e = kind.launch(p, q.variant, t->d_query_rays.get<float>(), t->d_query_hits.get<void>(), m, t->stream);
    if (e == hipSuccess) e = hipEventRecord(e1, t->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(static_cast<char*>(out) + (size_t)at * kind.out_bytes, t->d_query_hits.get<void>(),
                         (size_t)m * kind.out_bytes, hipMemcpyDeviceToHost, t->stream);
    // (a pageable host buffer makes each copy wait for its own completion; the buffers are reused chunk after
    // chunk in stream order either way)
  }
  if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
  t->host_waits++;
  if (e != hipSuccess) return HipFail(e, call);
  double ms = 0.0;
  for (size_t k = 0; k + 1 < ev.size(); k += 2) {
    float f = 0.0f;
    if (hipEventElapsedTime(&f, ev[k], ev[k + 1]) != hipSuccess) {
      ms = -1.0;
      break;
    }
    ms += (double)f;
  }
  t->query_pending = false;
  t->query_ms = ms;
  return RT2_OK;
}

// The device entry of either kind: two events around one launch, no wait.
int DeviceQuery(rt2_tracer* t, int64_t n, const float* d_rays, uint64_t seed, void* d_out, const QueryKind& kind,
                const char* call) {
  int rc = CheckCall(t, n, d_rays, d_out, call);
  if (rc != RT2_OK) return rc;
  if (n == 0) return RT2_OK;
  RenderParams p;
  QueryPlan q;
  if ((rc = QueryParams(t, seed, (uint32_t)n, call, &p, &q)) != RT2_OK) return rc;
  HIP_TRY(hipSetDevice(t->device));
  if (!t->query_e0 && hipEventCreate(&t->query_e0) != hipSuccess) return Fail(RT2_ERR_HIP, "event create failed");
  if (!t->query_e1 && hipEventCreate(&t->query_e1) != hipSuccess) return Fail(RT2_ERR_HIP, "event create failed");
  t->query_pending = false;
  t->query_ms = -1.0;
  HIP_TRY(hipEventRecord(t->query_e0, t->stream));
  HIP_TRY(kind.launch(p, q.variant, d_rays, d_out, (uint32_t)n, t->stream));
  HIP_TRY(hipEventRecord(t->query_e1, t->stream));
  t->query_pending = true;
  return RT2_OK;
}

// ---- ambient occlusion (rt2.h "Ambient occlusion", ambient.h) ----

// (the arguments first, as CheckCall: samples, then n and the pointers, then the tracer)
int CheckAmbient(const rt2_tracer* t, int samples, int64_t n, const void* points, const void* out, const char* call) {
  if (samples < 1 || samples > kAmbientMaxSamples)
    return Fail(RT2_ERR_INVALID, std::string(call) + ": need 1 <= samples <= 65535");
  return CheckCall(t, n, points, out, call);
}

// What an image call checks before it touches the device.
int CheckAmbientImage(const rt2_tracer* t, int samples, float radius, const void* out, const char* call) {
  if (!(radius > kQueryTmin) || !QueryFinite(radius))
    return Fail(RT2_ERR_INVALID, std::string(call) + ": need a finite radius above 0.001 (FLT_MAX: unbounded)");
  int rc = CheckAmbient(t, samples, 0, out, out, call);  // (no caller records: n and its pointer pass)
  if (rc != RT2_OK) return rc;
  if (t->comm) return Fail(RT2_ERR_INVALID, std::string(call) + ": not on a joined tracer (a set_partition tracer works)");
  if (t->width <= 0 || t->height <= 0) return Fail(RT2_ERR_INVALID, std::string(call) + ": no image yet (on_resize first)");
  return RT2_OK;
}

// Zeroes n words of d_counts and adds the samples' hits of n points of src into them: the plan's launches over
// consecutive sample ranges, all on the tracer's stream.
hipError_t EnqueueAmbient(const rt2_tracer* t, const RenderParams& p, const AmbientSource& src, uint32_t n, int samples,
                          uint32_t* d_counts) {
  const int variant = RenderVariant(t->features);
  const AmbientPlan a = PlanAmbient(p.lin_len, variant, RenderVariantFeatures(variant), p.stack_depth, n,
                                    (uint32_t)samples, RenderBlockSize());
  hipError_t e = hipMemsetAsync(d_counts, 0, (size_t)n * sizeof(uint32_t), t->stream);
  for (uint32_t l = 0; l < a.launches && e == hipSuccess; l++) {
    const uint32_t k = l + 1u == a.launches ? a.last : a.per_launch;
    e = LaunchAmbient(p, a.q.variant, src, n, l * a.per_launch, k, MakeMagic(k), d_counts, t->stream);
  }
  return e;
}

// The events of the device entries' last call (created at the first one), recorded around its kernels.
int AmbientEvents(rt2_tracer* t) {
  if (!t->ambient_e0 && hipEventCreate(&t->ambient_e0) != hipSuccess) return Fail(RT2_ERR_HIP, "event create failed");
  if (!t->ambient_e1 && hipEventCreate(&t->ambient_e1) != hipSuccess) return Fail(RT2_ERR_HIP, "event create failed");
  t->ambient_pending = false;
  t->ambient_ms = -1.0;
  return RT2_OK;
}

// A device entry's body: the events around the kernels over n points of src into d_out, no wait.
int DeviceAmbient(rt2_tracer* t, const RenderParams& p, const AmbientSource& src, uint32_t n, int samples,
                  uint32_t* d_out) {
  int rc = AmbientEvents(t);
  if (rc != RT2_OK) return rc;
  HIP_TRY(hipEventRecord(t->ambient_e0, t->stream));
  HIP_TRY(EnqueueAmbient(t, p, src, n, samples, d_out));
  HIP_TRY(hipEventRecord(t->ambient_e1, t->stream));
  t->ambient_pending = true;
  return RT2_OK;
}

// The image calls' points: the tracer's feature records under `seed`, traced on the stream if the cache is stale.
int ImageSource(rt2_tracer* t, float radius, uint64_t seed, AmbientSource* src) {
  const float* d_features = nullptr;
  int rc = FeaturesForSeed(t, seed, &d_features);
  if (rc != RT2_OK) return rc;
  *src = AmbientFeatureSource(d_features, radius, (uint32_t)t->width);
  return RT2_OK;
}

// The image's launch parameters: QueryParams and the tracer's partition (BaseParams has it), which the kernel's
// map from a local pixel to its global index reads.
int ImageParams(const rt2_tracer* t, uint64_t seed, const char* call, RenderParams* p) {
  QueryPlan q;
  return QueryParams(t, seed, 1u, call, p, &q);
}


// ---- radiance queries (rt2.h "Radiance queries", radiance.h) ----

// Most (ray, sample) items per launch: RT2_RADIANCE_ITEMS, read at every call, at most kRadianceItemsEnvMax (the slot
// buffer is allocated for a call's largest launch: 16 bytes per item).
uint32_t RadianceItemsMax() {
  if (const char* e = getenv("RT2_RADIANCE_ITEMS")) {
    const long long v = atoll(e);
    if (v > 0) return (uint32_t)std::min<long long>(v, (long long)kRadianceItemsEnvMax);
  }
  return kRadianceItemsDefault;
}
// RT2_RADIANCE_REFILL=0, read at every call: one item per lane (an A/B switch; the bytes are the same).
bool RadianceRefill() {
  const char* e = getenv("RT2_RADIANCE_REFILL");
  return !(e && e[0] == '0' && e[1] == '\0');
}

// (the arguments first, as CheckCall: the parameters, then n and the pointers, then the tracer); *a: the call's
// parameters with the defaults and the tracer's depth filled in
int CheckRadiance(const rt2_tracer* t, int64_t n, const void* rays, const uint32_t* host_streams,
                  const rt2_radiance_params* p, const void* out_sum, const char* call, RadianceArgs* a) {
  rt2_radiance_params d;
  rt2_radiance_defaults(&d);
  if (p) d = *p;
  if (!RadianceArgsValid(d.samples, d.max_depth, d.first_draw))
    return Fail(RT2_ERR_INVALID,
                std::string(call) + ": need 1 <= samples <= 65535, 0 <= max_depth <= 65535 and first_draw <= 8");
  // (host_streams: the host entry's stream words, whose frame words must leave room for the samples; with bad n or
  // pointers CheckCall below refuses first)
  if (host_streams && rays && out_sum && n > 0 && n < ((int64_t)1 << 31))
    for (int64_t i = 0; i < n; i++)
      if (!RadianceFrameFits(host_streams[2 * i + 1], (uint32_t)d.samples))
        return Fail(RT2_ERR_INVALID, std::string(call) + ": frame word + samples passes 2^32 at ray " + std::to_string(i));
  int rc = CheckCall(t, n, rays, out_sum, call);
  if (rc != RT2_OK) return rc;
  a->samples = (uint32_t)d.samples;
  a->max_depth = (uint32_t)(d.max_depth ? d.max_depth : t->max_depth);
  a->first_draw = d.first_draw;
  return RT2_OK;
}

// The plan's launches over n rays at d_rays (d_streams may be null; index0: the stream index of ray 0) onto d_sum
// and d_counts (may be null), all on the tracer's stream; grows the slot buffer to the plan's largest launch.
int EnqueueRadiance(rt2_tracer* t, const RenderParams& p, const float* d_rays, const uint32_t* d_streams,
                    uint32_t index0, uint32_t n, const RadianceArgs& a, float* d_sum, uint32_t* d_counts) {
  const int variant = RenderVariant(t->features);
  const int block = RenderBlockSize();
  const RadiancePlan r = PlanRadiance(p.lin_len, variant, RenderVariantFeatures(variant), p.stack_depth, n, a.samples,
                                      RadianceItemsMax(), block);
  const bool refill = RadianceRefill();
  const size_t slot_bytes = (size_t)r.rays_per_launch * r.per_launch * kRadianceSlotWords * sizeof(float);
  if (slot_bytes > t->d_radiance_slots.bytes()) {
    // (hipFree waits for the device: nothing queued still reads the old buffer)
    HIP_TRY(t->d_radiance_slots.Grow(slot_bytes));
    NoteDeviceBytes(t);
  }
  float* slots = t->d_radiance_slots.get<float>();
  for (uint32_t ra = 0; ra < r.ray_launches; ra++) {
    for (uint32_t sb = 0; sb < r.launches; sb++) {
      const RadianceLaunch l = RadianceLaunchAt(r, n, a.samples, ra, sb);
      const uint32_t items = l.rays * l.k, wave_items = RadianceWaveItems(items, refill);
      HIP_TRY(LaunchRadiance(p, r.q.variant, d_rays + (size_t)l.ray0 * kQueryRayFloats,
                             d_streams ? d_streams + 2u * (size_t)l.ray0 : nullptr, index0 + l.ray0, l.rays, l.s0, l.k,
                             MakeMagic(l.k), a, wave_items, RadianceGrid(items, wave_items, (uint32_t)block), slots,
                             d_sum + 3u * (size_t)l.ray0, d_counts ? d_counts + l.ray0 : nullptr, t->stream));
    }
  }
  return RT2_OK;
}

}  // namespace

extern "C" {

void rt2_radiance_defaults(rt2_radiance_params* p) {
  if (!p) return;
  p->samples = 1;
  p->max_depth = 0;
  p->first_draw = 0;
}

int rt2_tracer_radiance(rt2_tracer* t, int64_t n, const float* rays, const uint32_t* streams,
                        const rt2_radiance_params* params, uint64_t seed, float* out_sum, uint32_t* out_rays) {
  const char* call = "radiance";
  RadianceArgs a;
  int rc = CheckRadiance(t, n, rays, streams, params, out_sum, call, &a);
  if (rc != RT2_OK) return rc;
  if (n == 0) return RT2_OK;
  const int64_t chunk = std::min(QueryChunk(), (n + 63) / 64 * 64);
  RenderParams p;
  QueryPlan q;
  if ((rc = QueryParams(t, seed, 1u, call, &p, &q)) != RT2_OK) return rc;
  if ((rc = Flush(t)) != RT2_OK) return rc;  // queued frames first, as a readback does
  HIP_TRY(hipSetDevice(t->device));
  // rays and stream words in one buffer, sums and counts in the other
  const size_t ray_bytes = (size_t)chunk * kQueryRayFloats * sizeof(float);
  const size_t in_bytes = ray_bytes + (size_t)chunk * 2 * sizeof(uint32_t);
  const size_t sum_bytes = (size_t)chunk * 3 * sizeof(float);
  const size_t out_bytes = sum_bytes + (size_t)chunk * sizeof(uint32_t);
  if (in_bytes > t->d_query_rays.bytes() || out_bytes > t->d_query_hits.bytes()) {
    HIP_TRY(t->d_query_rays.Grow(in_bytes));
    HIP_TRY(t->d_query_hits.Grow(out_bytes));
    NoteDeviceBytes(t);
  }
  float* d_rays = t->d_query_rays.get<float>();
  uint32_t* d_streams = reinterpret_cast<uint32_t*>(t->d_query_rays.get<char>() + ray_bytes);
  float* d_sum = t->d_query_hits.get<float>();
  uint32_t* d_counts = reinterpret_cast<uint32_t*>(t->d_query_hits.get<char>() + sum_bytes);
  std::vector<hipEvent_t> ev;  // one pair per chunk, back to the tracer's pool on every way out
  struct Return {
    rt2_tracer* t;
    std::vector<hipEvent_t>& ev;
    ~Return() {
      for (hipEvent_t e : ev) t->event_pool.push_back(e);
    }
  } give_back{t, ev};
  hipError_t e = hipSuccess;
  for (int64_t at = 0; at < n && e == hipSuccess; at += chunk) {
    const uint32_t m = (uint32_t)std::min(chunk, n - at);
    hipEvent_t e0 = TakeEvent(t), e1 = TakeEvent(t);
    if (e0) ev.push_back(e0);
    if (e1) ev.push_back(e1);
    if (!e0 || !e1) return Fail(RT2_ERR_HIP, "event create failed");
    e = hipMemcpyAsync(d_rays, rays + (size_t)at * kQueryRayFloats, (size_t)m * kQueryRayFloats * sizeof(float),
                       hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess && streams)
      e = hipMemcpyAsync(d_streams, streams + 2 * (size_t)at, (size_t)m * 2 * sizeof(uint32_t), hipMemcpyHostToDevice,
                         t->stream);
    if (e == hipSuccess) e = hipEventRecord(e0, t->stream);
    if (e == hipSuccess) {
      rc = EnqueueRadiance(t, p, d_rays, streams ? d_streams : nullptr, (uint32_t)at, m, a, d_sum,
                           out_rays ? d_counts : nullptr);
      if (rc != RT2_OK) {
        (void)hipStreamSynchronize(t->stream);
        return rc;
      }
    }
    if (e == hipSuccess) e = hipEventRecord(e1, t->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(out_sum + 3 * (size_t)at, d_sum, (size_t)m * 3 * sizeof(float), hipMemcpyDeviceToHost, t->stream);
    if (e == hipSuccess && out_rays)
      e = hipMemcpyAsync(out_rays + at, d_counts, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost, t->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
  t->host_waits++;
  if (e != hipSuccess) return HipFail(e, call);
  double ms = 0.0;
  for (size_t k = 0; k + 1 < ev.size(); k += 2) {
    float f = 0.0f;
    if (hipEventElapsedTime(&f, ev[k], ev[k + 1]) != hipSuccess) {
      ms = -1.0;
      break;
    }
    ms += (double)f;
  }
  t->radiance_pending = false;
  t->radiance_ms = ms;
  return RT2_OK;
}

int rt2_tracer_radiance_device(rt2_tracer* t, int64_t n, const float* d_rays, const uint32_t* d_streams,
                               const rt2_radiance_params* params, uint64_t seed, float* d_out_sum,
                               uint32_t* d_out_rays) {
  const char* call = "radiance_device";
  RadianceArgs a;
  int rc = CheckRadiance(t, n, d_rays, nullptr, params, d_out_sum, call, &a);
  if (rc != RT2_OK) return rc;
  if (n == 0) return RT2_OK;
  RenderParams p;
  QueryPlan q;
  if ((rc = QueryParams(t, seed, 1u, call, &p, &q)) != RT2_OK) return rc;
  HIP_TRY(hipSetDevice(t->device));
  if (!t->radiance_e0 && hipEventCreate(&t->radiance_e0) != hipSuccess) return Fail(RT2_ERR_HIP, "event create failed");
  if (!t->radiance_e1 && hipEventCreate(&t->radiance_e1) != hipSuccess) return Fail(RT2_ERR_HIP, "event create failed");
  t->radiance_pending = false;
  t->radiance_ms = -1.0;
  HIP_TRY(hipEventRecord(t->radiance_e0, t->stream));
  if ((rc = EnqueueRadiance(t, p, d_rays, d_streams, 0u, (uint32_t)n, a, d_out_sum, d_out_rays)) != RT2_OK) return rc;
  HIP_TRY(hipEventRecord(t->radiance_e1, t->stream));
  t->radiance_pending = true;
  return RT2_OK;
}

int rt2_tracer_radiance_time(rt2_tracer* t, double* ms) {
  if (!t || !ms) return Fail(RT2_ERR_INVALID, "radiance_time: null argument");
  if (IsMulti(t)) return Fail(RT2_ERR_INVALID, "radiance_time: not on a create_multi tracer");
  if (t->radiance_pending) {
    HIP_TRY(hipSetDevice(t->device));
    const hipError_t q = hipEventQuery(t->radiance_e1);
    if (q == hipSuccess) {
      float f = -1.0f;
      if (hipEventElapsedTime(&f, t->radiance_e0, t->radiance_e1) != hipSuccess) f = -1.0f;
      t->radiance_ms = (double)f;
      t->radiance_pending = false;
    } else if (q != hipErrorNotReady) {
      return HipFail(q, "radiance_time");
    }
  }
  *ms = t->radiance_pending ? -1.0 : t->radiance_ms;
  return RT2_OK;
}

int rt2_ambient_direction(const float* n3, const float* u3, float* d3) {
  if (!n3 || !u3 || !d3) return Fail(RT2_ERR_INVALID, "ambient_direction: null pointer");
  AmbientDirection(n3, u3, d3);
  return RT2_OK;
}

int rt2_tracer_ambient(rt2_tracer* t, int samples, float radius, uint64_t seed, uint32_t* out) {
  const char* call = "ambient";
  int rc = CheckAmbientImage(t, samples, radius, out, call);
  if (rc != RT2_OK) return rc;
  const size_t n = (size_t)t->width * (size_t)t->local_rows;
  if (n == 0) return RT2_OK;
  RenderParams p;
  if ((rc = ImageParams(t, seed, call, &p)) != RT2_OK) return rc;
  if ((rc = Flush(t)) != RT2_OK) return rc;  // queued frames first, as a readback does
  HIP_TRY(hipSetDevice(t->device));
  AmbientSource src;
  if ((rc = ImageSource(t, radius, seed, &src)) != RT2_OK) return rc;
  if (n * sizeof(uint32_t) > t->d_query_hits.bytes()) {
    HIP_TRY(t->d_query_hits.Grow(n * sizeof(uint32_t)));
    NoteDeviceBytes(t);
  }
  EventPair ev(t);
  if (!ev.Take()) return Fail(RT2_ERR_HIP, "event create failed");
  uint32_t* d_counts = t->d_query_hits.get<uint32_t>();
  hipError_t e = hipEventRecord(ev.e0, t->stream);
  if (e == hipSuccess) e = EnqueueAmbient(t, p, src, (uint32_t)n, samples, d_counts);
  if (e == hipSuccess) e = hipEventRecord(ev.e1, t->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_counts, n * sizeof(uint32_t), hipMemcpyDeviceToHost, t->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
  t->host_waits++;
  if (e != hipSuccess) return HipFail(e, call);
  float f = -1.0f;
  if (hipEventElapsedTime(&f, ev.e0, ev.e1) != hipSuccess) f = -1.0f;
  t->ambient_pending = false;
  t->ambient_ms = (double)f;
  return RT2_OK;
}

int rt2_tracer_ambient_device(rt2_tracer* t, int samples, float radius, uint64_t seed, uint32_t* d_out) {
  const char* call = "ambient_device";
  int rc = CheckAmbientImage(t, samples, radius, d_out, call);
  if (rc != RT2_OK) return rc;
  const size_t n = (size_t)t->width * (size_t)t->local_rows;
  if (n == 0) return RT2_OK;
  RenderParams p;
  if ((rc = ImageParams(t, seed, call, &p)) != RT2_OK) return rc;
  HIP_TRY(hipSetDevice(t->device));
  AmbientSource src;
  if ((rc = ImageSource(t, radius, seed, &src)) != RT2_OK) return rc;
  return DeviceAmbient(t, p, src, (uint32_t)n, samples, d_out);
}

int rt2_tracer_ambient_points(rt2_tracer* t, int64_t n, const float* points, int samples, uint64_t seed, uint32_t* out) {
  const char* call = "ambient_points";
  int rc = CheckAmbient(t, samples, n, points, out, call);
  if (rc != RT2_OK) return rc;
  if (n == 0) return RT2_OK;
  const int64_t chunk = std::min(QueryChunk(), (n + 63) / 64 * 64);
  RenderParams p;
  QueryPlan q;
  if ((rc = QueryParams(t, seed, 1u, call, &p, &q)) != RT2_OK) return rc;
  if ((rc = Flush(t)) != RT2_OK) return rc;  // queued frames first, as a readback does
  HIP_TRY(hipSetDevice(t->device));
  const size_t in_bytes = (size_t)chunk * kQueryRayFloats * sizeof(float);
  const size_t out_bytes = (size_t)chunk * sizeof(uint32_t);
  if (in_bytes > t->d_query_rays.bytes() || out_bytes > t->d_query_hits.bytes()) {
    HIP_TRY(t->d_query_rays.Grow(in_bytes));
    HIP_TRY(t->d_query_hits.Grow(out_bytes));
    NoteDeviceBytes(t);
  }
  std::vector<hipEvent_t> ev;  // one pair per chunk, back to the tracer's pool on every way out
  struct Return {
    rt2_tracer* t;
    std::vector<hipEvent_t>& ev;
    ~Return() {
      for (hipEvent_t e : ev) t->event_pool.push_back(e);
    }
  } give_back{t, ev};
  uint32_t* d_counts = t->d_query_hits.get<uint32_t>();
  hipError_t e = hipSuccess;
  for (int64_t at = 0; at < n && e == hipSuccess; at += chunk) {
    const uint32_t m = (uint32_t)std::min(chunk, n - at);
    hipEvent_t e0 = TakeEvent(t), e1 = TakeEvent(t);
    if (e0) ev.push_back(e0);
    if (e1) ev.push_back(e1);
    if (!e0 || !e1) return Fail(RT2_ERR_HIP, "event create failed");
    e = hipMemcpyAsync(t->d_query_rays.get<float>(), points + (size_t)at * kQueryRayFloats,
                       (size_t)m * kQueryRayFloats * sizeof(float), hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess) e = hipEventRecord(e0, t->stream);
    if (e == hipSuccess)
      e = EnqueueAmbient(t, p, AmbientRecordSource(t->d_query_rays.get<float>(), (uint32_t)at), m, samples, d_counts);
    if (e == hipSuccess) e = hipEventRecord(e1, t->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(out + at, d_counts, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost, t->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
  t->host_waits++;
  if (e != hipSuccess) return HipFail(e, call);
  double ms = 0.0;
  for (size_t k = 0; k + 1 < ev.size(); k += 2) {
    float f = 0.0f;
    if (hipEventElapsedTime(&f, ev[k], ev[k + 1]) != hipSuccess) {
      ms = -1.0;
      break;
    }
    ms += (double)f;
  }
  t->ambient_pending = false;
  t->ambient_ms = ms;
  return RT2_OK;
}

int rt2_tracer_ambient_points_device(rt2_tracer* t, int64_t n, const float* d_points, int samples, uint64_t seed,
                                     uint32_t* d_out) {
  const char* call = "ambient_points_device";
  int rc = CheckAmbient(t, samples, n, d_points, d_out, call);
  if (rc != RT2_OK) return rc;
  if (n == 0) return RT2_OK;
  RenderParams p;
  QueryPlan q;
  if ((rc = QueryParams(t, seed, 1u, call, &p, &q)) != RT2_OK) return rc;
  HIP_TRY(hipSetDevice(t->device));
  return DeviceAmbient(t, p, AmbientRecordSource(d_points, 0u), (uint32_t)n, samples, d_out);
}

int rt2_tracer_ambient_time(rt2_tracer* t, double* ms) {
  if (!t || !ms) return Fail(RT2_ERR_INVALID, "ambient_time: null argument");
  if (IsMulti(t)) return Fail(RT2_ERR_INVALID, "ambient_time: not on a create_multi tracer");
  if (t->ambient_pending) {
    HIP_TRY(hipSetDevice(t->device));
    const hipError_t q = hipEventQuery(t->ambient_e1);
    if (q == hipSuccess) {
      float f = -1.0f;
      if (hipEventElapsedTime(&f, t->ambient_e0, t->ambient_e1) != hipSuccess) f = -1.0f;
      t->ambient_ms = (double)f;
      t->ambient_pending = false;
    } else if (q != hipErrorNotReady) {
      return HipFail(q, "ambient_time");
    }
  }
  *ms = t->ambient_pending ? -1.0 : t->ambient_ms;
  return RT2_OK;
}

int rt2_query_ray_valid(const float* ray8) { return ray8 && QueryRayValid(ray8) ? 1 : 0; }

int rt2_tracer_intersect(rt2_tracer* t, int64_t n, const float* rays, uint64_t seed, float* out) {
  return HostQuery(t, n, rays, seed, out, kClosestHit, "intersect");
}

int rt2_tracer_intersect_device(rt2_tracer* t, int64_t n, const float* d_rays, uint64_t seed, float* d_out) {
  return DeviceQuery(t, n, d_rays, seed, d_out, kClosestHit, "intersect_device");
}

int rt2_tracer_occluded(rt2_tracer* t, int64_t n, const float* rays, uint64_t seed, int8_t* out) {
  return HostQuery(t, n, rays, seed, out, kOcclusion, "occluded");
}

int rt2_tracer_occluded_device(rt2_tracer* t, int64_t n, const float* d_rays, uint64_t seed, int8_t* d_out) {
  return DeviceQuery(t, n, d_rays, seed, d_out, kOcclusion, "occluded_device");
}

int rt2_tracer_intersect_time(rt2_tracer* t, double* ms) {
  if (!t || !ms) return Fail(RT2_ERR_INVALID, "intersect_time: null argument");
  if (IsMulti(t)) return Fail(RT2_ERR_INVALID, "intersect_time: not on a create_multi tracer");
  if (t->query_pending) {
    HIP_TRY(hipSetDevice(t->device));
    const hipError_t q = hipEventQuery(t->query_e1);
    if (q == hipSuccess) {
      float f = -1.0f;
      if (hipEventElapsedTime(&f, t->query_e0, t->query_e1) != hipSuccess) f = -1.0f;
      t->query_ms = (double)f;
      t->query_pending = false;
    } else if (q != hipErrorNotReady) {
      return HipFail(q, "intersect_time");
    }
  }
  *ms = t->query_pending ? -1.0 : t->query_ms;
  return RT2_OK;
}

}  // extern "C"
