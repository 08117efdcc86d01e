// capi_query.cpp — the ray queries of include/rt2.h ("Ray queries"): the scene's closest Hit for rays the caller
// owns, over render.hip's query kernel, and whether anything is in their way, over its occlusion kernel. Planned by launch_plan.h PlanQuery; the layouts and the validity rule are
// query.h's. And "Ambient occlusion": blocked-sample counts per pixel or caller point over render.hip's ambient
// kernel, through the same buffers and chunks; planned by PlanAmbient, the rule is ambient.h's. And "Radiance
// queries": RayColorForward along the caller's rays over render.hip's radiance kernels, through the same buffers and
// chunks and a slot buffer; planned by PlanRadiance, the rule is radiance.h's.
//
// Every family has the same two ways in. A host entry checks its arguments, builds its parameters, launches the queued
// frames and hands ChunkedHostCall its spans and what to enqueue per chunk: the buffers, the borrowed events, the
// copies, the one wait, host_waits and the family's timer are that function's. A device entry brackets one enqueue
// with its family's KernelTimer (tracer.h) and does not wait; its _time export polls that timer.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdlib>
#include <initializer_list>
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

// One span of a chunked host call: `host` holds item_bytes per item of the whole call (null: nothing is copied, the
// room stays), and a chunk's items lie `offset` bytes into the device buffer: d_query_rays for the inputs,
// d_query_hits for the outputs.
struct InSpan {
  const void* host;
  size_t item_bytes, offset;
};
struct OutSpan {
  void* host;
  size_t item_bytes, offset;
};
template <typename Span>
size_t SpanBytes(std::initializer_list<Span> spans, int64_t chunk) {  // what a chunk of them needs of its buffer
  size_t bytes = 0;
  for (const Span& s : spans) bytes = std::max(bytes, s.offset + (size_t)chunk * s.item_bytes);
  return bytes;
}

// The chunk of a host entry over n items: QueryChunk(), or n's whole waves where that is less.
int64_t CallChunk(int64_t n) { return std::min(QueryChunk(), (n + 63) / 64 * 64); }

// The body of every host entry, after its checks, its parameters and Flush: n > 0 items in chunks of `chunk` through
// the tracer's two query buffers (both grown when either is too small, and kept). Per chunk the inputs are copied
// in, enqueue(at, m, &refusal) puts the kernels of items [at, at + m) on the tracer's stream between two events borrowed
// from the tracer's pool (back in it on every way out), and the outputs are copied out; then one wait, and the
// events' times summed into `timer`. enqueue returns HIP's answer, or sets refusal to a code of its own, already
// reported: the call then waits for what is queued and returns it.
// (a pageable host buffer makes each copy wait for its own completion; the buffers are reused chunk after chunk in
// stream order either way)
template <typename Enqueue>
int ChunkedHostCall(rt2_tracer* t, const char* call, KernelTimer& timer, int64_t n, int64_t chunk,
                    std::initializer_list<InSpan> in, std::initializer_list<OutSpan> out, Enqueue&& enqueue) {
  HIP_TRY(hipSetDevice(t->device));
  const size_t in_bytes = SpanBytes(in, chunk), out_bytes = SpanBytes(out, chunk);
  if (in_bytes > t->d_query_rays.bytes() || out_bytes > t->d_query_hits.bytes()) {
    // (hipFree waits for the device: nothing queued still reads the old buffers)
    HIP_TRY(t->d_query_rays.Grow(in_bytes));
    HIP_TRY(t->d_query_hits.Grow(out_bytes));
    NoteDeviceBytes(t);
  }
  struct Borrowed {
    rt2_tracer* t;
    std::vector<hipEvent_t> ev;  // e0, e1 of each chunk
    ~Borrowed() {
      for (hipEvent_t e : ev) t->event_pool.push_back(e);
    }
  } pairs{t, {}};
  char* const d_in = t->d_query_rays.get<char>();
  char* const d_out = t->d_query_hits.get<char>();
  hipError_t e = hipSuccess;
  for (int64_t at = 0; at < n && e == hipSuccess; at += chunk) {
    const uint32_t m = (uint32_t)std::min(chunk, n - at);
    hipEvent_t e0 = TakeEvent(t), e1 = TakeEvent(t);
    if (e0) pairs.ev.push_back(e0);
    if (e1) pairs.ev.push_back(e1);
    if (!e0 || !e1) return Fail(RT2_ERR_HIP, "event create failed");
    for (const InSpan& s : in)
      if (e == hipSuccess && s.host)
        e = hipMemcpyAsync(d_in + s.offset, static_cast<const char*>(s.host) + (size_t)at * s.item_bytes,
                           (size_t)m * s.item_bytes, hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess) e = hipEventRecord(e0, t->stream);
    if (e == hipSuccess) {
      int rc = RT2_OK;
      e = enqueue(at, m, &rc);
      if (rc != RT2_OK) {
        (void)hipStreamSynchronize(t->stream);
        return rc;
      }
    }
    if (e == hipSuccess) e = hipEventRecord(e1, t->stream);
    for (const OutSpan& s : out)
      if (e == hipSuccess && s.host)
        e = hipMemcpyAsync(static_cast<char*>(s.host) + (size_t)at * s.item_bytes, d_out + s.offset,
                           (size_t)m * s.item_bytes, hipMemcpyDeviceToHost, t->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
  t->host_waits++;
  if (e != hipSuccess) return HipFail(e, call);
  double ms = 0.0;
  for (size_t k = 0; k + 1 < pairs.ev.size(); k += 2) {
    float f = 0.0f;
    if (hipEventElapsedTime(&f, pairs.ev[k], pairs.ev[k + 1]) != hipSuccess) {
      ms = -1.0;
      break;
    }
    ms += (double)f;
  }
  timer.Set(ms);
  return RT2_OK;
}

// The host entry of either kind. The record buffer is sized for the closest hit's records whichever the kind (they
// hold an occlusion chunk's bytes 64 times over): the span without a host pointer says so.
int HostQuery(rt2_tracer* t, int64_t n, const float* rays, uint64_t seed, void* out, const QueryKind& kind,
              const char* call) {
  int rc = CheckCall(t, n, rays, out, call);
  if (rc != RT2_OK) return rc;
  if (n == 0) return RT2_OK;
  const int64_t chunk = CallChunk(n);
  RenderParams p;
  QueryPlan q;
  if ((rc = QueryParams(t, seed, (uint32_t)std::min(chunk, n), call, &p, &q)) != RT2_OK) return rc;
  if ((rc = Flush(t)) != RT2_OK) return rc;  // queued frames first, as a readback does
  return ChunkedHostCall(t, call, t->query_timer, n, chunk, {{rays, kQueryRayFloats * sizeof(float), 0}},
                         {{out, kind.out_bytes, 0}, {nullptr, kQueryHitFloats * sizeof(float), 0}},
                         [&](int64_t, uint32_t m, int*) {
                           return kind.launch(p, q.variant, t->d_query_rays.get<float>(), t->d_query_hits.get<void>(), m,
                                              t->stream);
                         });
}

// The device entry of either kind: the timer around one launch, no wait.
int DeviceQuery(rt2_tracer* t, int64_t n, const float* d_rays, uint64_t seed, void* d_out, const QueryKind& kind,
                const char* call) {
  int rc = CheckCall(t, n, d_rays, d_out, call);
  if (rc != RT2_OK) return rc;
  if (n == 0) return RT2_OK;
  RenderParams p;
  QueryPlan q;
  if ((rc = QueryParams(t, seed, (uint32_t)n, call, &p, &q)) != RT2_OK) return rc;
  HIP_TRY(hipSetDevice(t->device));
  if ((rc = t->query_timer.Begin(t->stream)) != RT2_OK) return rc;
  HIP_TRY(kind.launch(p, q.variant, d_rays, d_out, (uint32_t)n, t->stream));
  return t->query_timer.End(t->stream);
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

// A device entry's body: the timer around the kernels over n points of src into d_out, no wait.
int DeviceAmbient(rt2_tracer* t, const RenderParams& p, const AmbientSource& src, uint32_t n, int samples,
                  uint32_t* d_out) {
  int rc = t->ambient_timer.Begin(t->stream);
  if (rc != RT2_OK) return rc;
  HIP_TRY(EnqueueAmbient(t, p, src, n, samples, d_out));
  return t->ambient_timer.End(t->stream);
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
  const int64_t chunk = CallChunk(n);
  RenderParams p;
  QueryPlan q;
  if ((rc = QueryParams(t, seed, 1u, call, &p, &q)) != RT2_OK) return rc;
  if ((rc = Flush(t)) != RT2_OK) return rc;  // queued frames first, as a readback does
  // rays and stream words in one buffer, sums and counts in the other
  const size_t ray_bytes = (size_t)chunk * kQueryRayFloats * sizeof(float);
  const size_t sum_bytes = (size_t)chunk * 3 * sizeof(float);
  return ChunkedHostCall(
      t, call, t->radiance_timer, n, chunk,
      {{rays, kQueryRayFloats * sizeof(float), 0}, {streams, 2 * sizeof(uint32_t), ray_bytes}},
      {{out_sum, 3 * sizeof(float), 0}, {out_rays, sizeof(uint32_t), sum_bytes}}, [&](int64_t at, uint32_t m, int* refusal) {
        char* d_in = t->d_query_rays.get<char>();
        char* d_out = t->d_query_hits.get<char>();
        *refusal = EnqueueRadiance(t, p, reinterpret_cast<float*>(d_in),
                                   streams ? reinterpret_cast<uint32_t*>(d_in + ray_bytes) : nullptr, (uint32_t)at, m, a,
                                   reinterpret_cast<float*>(d_out),
                                   out_rays ? reinterpret_cast<uint32_t*>(d_out + sum_bytes) : nullptr);
        return hipSuccess;
      });
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
  if ((rc = t->radiance_timer.Begin(t->stream)) != RT2_OK) return rc;
  if ((rc = EnqueueRadiance(t, p, d_rays, d_streams, 0u, (uint32_t)n, a, d_out_sum, d_out_rays)) != RT2_OK) return rc;
  return t->radiance_timer.End(t->stream);
}

int rt2_tracer_radiance_time(rt2_tracer* t, double* ms) {
  if (!t || !ms) return Fail(RT2_ERR_INVALID, "radiance_time: null argument");
  if (IsMulti(t)) return Fail(RT2_ERR_INVALID, "radiance_time: not on a create_multi tracer");
  return t->radiance_timer.Poll(t->device, "radiance_time", ms);
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
  // one chunk of its n pixels, with nothing to copy in
  return ChunkedHostCall(t, call, t->ambient_timer, (int64_t)n, (int64_t)n, {}, {{out, sizeof(uint32_t), 0}},
                         [&](int64_t, uint32_t m, int*) {
                           return EnqueueAmbient(t, p, src, m, samples, t->d_query_hits.get<uint32_t>());
                         });
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
  RenderParams p;
  QueryPlan q;
  if ((rc = QueryParams(t, seed, 1u, call, &p, &q)) != RT2_OK) return rc;
  if ((rc = Flush(t)) != RT2_OK) return rc;  // queued frames first, as a readback does
  return ChunkedHostCall(t, call, t->ambient_timer, n, CallChunk(n), {{points, kQueryRayFloats * sizeof(float), 0}},
                         {{out, sizeof(uint32_t), 0}}, [&](int64_t at, uint32_t m, int*) {
                           return EnqueueAmbient(t, p, AmbientRecordSource(t->d_query_rays.get<float>(), (uint32_t)at), m,
                                                 samples, t->d_query_hits.get<uint32_t>());
                         });
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
  return t->ambient_timer.Poll(t->device, "ambient_time", ms);
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
  return t->query_timer.Poll(t->device, "intersect_time", ms);
}

}  // extern "C"
