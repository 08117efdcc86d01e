// capi_filter.cpp — the feature buffers, the denoiser, temporal reuse and the presenting calls of include/rt2.h
// (over render.hip's feature pass, denoise.hip, temporal.hip and present.hip).
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>
#include <string>

#include "tracer.h"

using namespace rt2;
using namespace rt2::detail;

// ---- what the calls below share: refusals, parameters, the chain, the feature pass, the way back to the host ----
// The local calls run on a tracer that holds the whole image on one GPU.
static bool OneGpu(const rt2_tracer* t) { return !IsMulti(t) && !t->comm && t->world == 1; }

// The refusals several calls share, each under the call's own prefix ("denoise", "temporal", "present").
static int OneGpuRefusal(const char* call) {
  return Fail(RT2_ERR_INVALID, std::string(call) + ": needs an unpartitioned one-GPU tracer (world 1, not joined)");
}
static int MomentsRefusal(const char* call) {
  return Fail(RT2_ERR_INVALID, std::string(call) + ": moments not enabled (rt2_tracer_enable_moments)");
}
static int FramesRefusal(const char* call) { return Fail(RT2_ERR_INVALID, std::string(call) + " needs at least 2 frames"); }

// The feature pass runs the stack traversal: a scene only the threaded program can render is refused.
static int StackRefusal(const rt2_tracer* t) {
  return Fail(RT2_ERR_INVALID, "features: the scene needs a traversal stack of " + std::to_string(t->max_stack) +
                                   " entries (kernel has " + std::to_string(kTraversalStack) + ")");
}

static int DenoiseParamsOf(const rt2_denoise_params* p, DenoiseParams* k) {
  *k = DenoiseDefaults();
  if (p) *k = DenoiseParams{p->iterations, p->normal_power_log2, p->sigma_l, p->sigma_p, p->sigma_a, p->eps_l};
  if (!DenoiseParamsValid(*k))
    return Fail(RT2_ERR_INVALID, "denoise: need 1 <= iterations <= 8, 0 <= normal_power_log2 <= 8, and sigma_l, sigma_p, "
                                 "sigma_a, eps_l finite and > 0");
  return RT2_OK;
}

static int TemporalParamsOf(const rt2_temporal_params* p, TemporalParams* k) {
  *k = TemporalDefaults();
  if (p) *k = TemporalParams{p->max_history, p->max_history_specular, p->min_normal_dot, p->sigma_p, p->sigma_a};
  if (!TemporalParamsValid(*k))
    return Fail(RT2_ERR_INVALID, "temporal: need max_history, sigma_p, sigma_a finite and > 0, max_history_specular finite "
                                 "and >= 0, min_normal_dot finite");
  return RT2_OK;
}

// The stages a rt2_present_params switches on and their parameters, checked only for those stages.
struct PresentStages {
  bool temporal = true, denoise = true;
  TemporalParams tk = TemporalDefaults();
  DenoiseParams dk = DenoiseDefaults();
};
static int PresentStagesOf(const rt2_present_params* params, PresentStages* s) {
  int rc;
  if (params) {
    s->temporal = params->temporal != 0;
    s->denoise = params->denoise != 0;
  }
  if (s->temporal && (rc = TemporalParamsOf(params ? &params->tp : nullptr, &s->tk)) != RT2_OK) return rc;
  if (s->denoise && (rc = DenoiseParamsOf(params ? &params->dp : nullptr, &s->dk)) != RT2_OK) return rc;
  return RT2_OK;
}

// The small steps' LDS tiles (denoise.hip): on unless RT2_DENOISE_LDS=0 (measured: DESIGN.md §6e).
static bool DenoiseLds() {
  const char* e = getenv("RT2_DENOISE_LDS");
  return !(e && e[0] == '0');
}

// GPU time between the pair's events, recorded on the tracer's stream, which the caller has synchronised.
static double EventMs(const EventPair& ev) {
  float ms = -1.0f;
  if (hipEventElapsedTime(&ms, ev.e0, ev.e1) != hipSuccess) ms = -1.0f;
  return (double)ms;
}

// What the reconstruction chain (inputs, temporal blend, filter, tone map) runs over: a one-GPU tracer's local
// image, or the gathered image on its root (rt2.h "Reconstructing the gathered image"). The kernels take
// pointers and dimensions, so the two differ only in which Recon of the tracer they use, in the rows, and in where
// the estimate comes from.
struct Chain {
  rt2_tracer* t;  // device, stream, material table, event pool
  Recon& recon;   // features (current), scratch, history, present timer
  int width, rows;
  int64_t frames;
  // the estimate: the sums (LaunchDenoiseInputs divides and takes the variance; counts: adaptive sampling's, or
  // null), or with accum null the resolved colour and variance of the mean (the gather's kernel has done both;
  // they are copied; counts: the gathered n_p when the ranks sent them, the blend's lengths, or null)
  const float *accum = nullptr, *moment2 = nullptr;
  const uint32_t* counts = nullptr;
  const float *color = nullptr, *variance = nullptr;
  Chain(rt2_tracer* tracer, Recon& r, int w, int h, int64_t f) : t(tracer), recon(r), width(w), rows(h), frames(f) {}
  size_t n() const { return (size_t)width * (size_t)rows; }
  float* head() const { return recon.d_scratch.get<float>(); }  // colour float3, then the variance of the mean
  const float* features() const { return recon.d_features.get<float>(); }
};

static Chain LocalChain(rt2_tracer* t) {
  Chain c(t, t->recon, t->width, t->local_rows, t->frame_idx);
  c.accum = t->d_accum.get<float>();
  c.moment2 = t->d_moment2.get<float>();
  if (t->adaptive_on) c.counts = t->d_counts.get<uint32_t>();
  return c;
}

// The gathered image on its root r, whose estimate (rt2_tracer_gather_estimate) is current.
static Chain ImageChain(rt2_tracer* r) {
  Chain c(r, r->image_recon, r->width, r->height, r->estimate_frame);
  c.color = r->d_image_nc.get<float>();
  c.variance = r->d_image_var.get<float>();
  // gathered with the ranks' sample counts (adaptive sampling of the gathered image): the gather's kernel divided
  // by each pixel's own n_p, and the blend's length is that n_p, as in LocalChain
  if (r->image_counts) c.counts = r->d_image_n.get<uint32_t>();
  return c;
}

// The part of the image a feature pass traces (the RenderParams fields of these names).
struct Partition {
  int local_rows, band_h, rank, world;
};

// The feature records of `part` of the tracer's image in rc, on the tracer's device, traced again when the camera
// or the seed have changed since (a change of size or partition drops the buffer: Realloc, FreeImage).
// alloc_pixels: the records the buffer is allocated for. seed: the pass's (the tracer's, or an ambient call's). ev:
// events recorded around the pass, or null; launched (or null): whether a pass ran. Enqueued on the tracer's stream;
// the host does not wait.
static int EnsureFeatures(rt2_tracer* t, Recon& rc, const Partition& part, size_t alloc_pixels, uint64_t seed,
                          const EventPair* ev, bool* launched) {
  if (launched) *launched = false;
  if (!t->stack_ok) return StackRefusal(t);
  const size_t n = (size_t)t->width * (size_t)part.local_rows;
  const CameraParams cam = t->camera.Params();
  if (n == 0) return RT2_OK;
  if (rc.d_features && rc.features_valid && rc.features_seed == seed && memcmp(&rc.features_cam, &cam, sizeof(cam)) == 0)
    return RT2_OK;
  HIP_TRY(hipSetDevice(t->device));
  if (!rc.d_features) {
    HIP_TRY(rc.d_features.Alloc(alloc_pixels * kDenoiseFeatureFloats * sizeof(float)));
    NoteDeviceBytes(t);
  }
  RenderParams p;
  BaseParams(t, cam, &p);
  p.local_rows = part.local_rows;
  p.band_h = part.band_h;
  p.rank = part.rank;
  p.world = part.world;
  p.local_pixels = (uint32_t)n;
  p.seed_lo = (uint32_t)seed;  // (BaseParams took the tracer's)
  p.seed_hi = (uint32_t)(seed >> 32);
  for (uint32_t r = 0; r < 10; r++) {
    p.philox_keys[2 * r] = p.seed_lo + r * 0x9E3779B9u;
    p.philox_keys[2 * r + 1] = p.seed_hi + r * 0xBB67AE85u;
  }
  if (ev) HIP_TRY(hipEventRecord(ev->e0, t->stream));
  HIP_TRY(LaunchFeatures(p, rc.d_features.get<float>(), t->stream));
  if (ev) HIP_TRY(hipEventRecord(ev->e1, t->stream));
  rc.features_valid = true;
  rc.features_cam = cam;
  rc.features_seed = seed;
  if (launched) *launched = true;
  return RT2_OK;
}

// The tracer's own band, as BaseParams describes it; the buffer is as tall as the accumulation.
static int LocalFeatures(rt2_tracer* t, uint64_t seed, const EventPair* ev, bool* launched) {
  const Partition own{t->local_rows, t->band_h > 0 ? t->band_h : t->height, t->rank, t->world};
  return EnsureFeatures(t, t->recon, own, (size_t)t->width * (size_t)AllocRows(t), seed, ev, launched);
}
static int LocalFeatures(rt2_tracer* t, const EventPair* ev, bool* launched) {
  return LocalFeatures(t, t->seed, ev, launched);
}

// (tracer.h) For rt2_tracer_ambient: the local records as traced under `seed`, no events and no wait.
int rt2::detail::FeaturesForSeed(rt2_tracer* t, uint64_t seed, const float** d_features) {
  int rc = LocalFeatures(t, seed, nullptr, nullptr);
  if (rc == RT2_OK) *d_features = t->recon.d_features.get<float>();
  return rc;
}

// The whole image on the root of a gathered image. The root traces every pixel itself: with world 1, rank 0 and
// one band of the image's height, features_kernel's map from local to image rows is the identity.
static int ImageFeatures(rt2_tracer* r) {
  const Partition whole{r->height, r->height, 0, 1};
  return EnsureFeatures(r, r->image_recon, whole, (size_t)r->width * (size_t)r->height, r->seed, nullptr, nullptr);
}

static int FeaturesTimed(rt2_tracer* t) {
  EventPair ev(t);
  if (!ev.Take()) return Fail(RT2_ERR_HIP, "event create failed");
  bool launched = false;
  int rc = LocalFeatures(t, &ev, &launched);
  if (rc != RT2_OK || !launched) return rc;
  hipError_t e = hipStreamSynchronize(t->stream);
  t->host_waits++;
  if (e != hipSuccess) return HipFail(e, "feature pass");
  t->features_ms = EventMs(ev);
  return RT2_OK;
}

// What rt2_tracer_denoise and the temporal calls need of a one-GPU tracer after their own checks: moments, every
// frame launched and finished, two frames, current features (timed).
static int LocalEstimateReady(rt2_tracer* t, const char* call) {
  if (!t->moments_on) return MomentsRefusal(call);
  int rc = Sync(t);
  if (rc != RT2_OK) return rc;
  if (t->frame_idx < 2) return FramesRefusal(call);
  return FeaturesTimed(t);
}

// rc's n feature records, copied to the host.
static int ReadFeatures(rt2_tracer* t, const Recon& rc, size_t n, float* out) {
  if (n == 0) return RT2_OK;
  HIP_TRY(hipSetDevice(t->device));
  HIP_TRY(hipMemcpyAsync(out, rc.d_features.get<float>(), n * kDenoiseFeatureFloats * sizeof(float), hipMemcpyDeviceToHost,
                         t->stream));
  t->host_waits++;
  HIP_TRY(hipStreamSynchronize(t->stream));
  return RT2_OK;
}

// The way back to the host of every resolve: after the enqueues so far (e: their result), copies the resolved
// colour and, where the pointers are not null, the variance behind it (d_color: a scratch's head) and the length
// plane d_len, then waits for the stream. waits: the tracer's host_waits, or null (no tracer). An error is
// reported under the call's name.
static int ReadBack(hipError_t e, const float* d_color, const float* d_len, size_t n, float* out_color, float* out_variance,
                    float* out_length, hipStream_t stream, uint64_t* waits, const char* call) {
  if (e == hipSuccess) e = hipMemcpyAsync(out_color, d_color, n * 3 * sizeof(float), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess && out_variance)
    e = hipMemcpyAsync(out_variance, d_color + 3 * n, n * sizeof(float), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess && out_length) e = hipMemcpyAsync(out_length, d_len, n * sizeof(float), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (waits) ++*waits;
  if (e != hipSuccess) return HipFail(e, call);
  return RT2_OK;
}

// What the *_buffers calls share: the checks of the image's size and of the device under the call's name, the
// device made current, and a non-blocking stream that lasts as long as this object. Declared after the call's
// DeviceBuffers: the stream goes before they are freed.
struct BufferCall {
  hipStream_t stream = nullptr;
  BufferCall() = default;
  BufferCall(const BufferCall&) = delete;
  BufferCall& operator=(const BufferCall&) = delete;
  ~BufferCall() {
    if (stream) (void)hipStreamDestroy(stream);
  }
  static int CheckSize(const char* call, int width, int height) {
    if (width <= 0 || height <= 0 || (int64_t)width * height >= (int64_t)1 << 26)
      return Fail(RT2_ERR_INVALID, std::string(call) + ": need width, height > 0 and width * height below 2^26");
    return RT2_OK;
  }
  int Open(const char* call, int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return Fail(RT2_ERR_HIP, "no HIP device available");
    if (device < 0 || device >= ndev) return Fail(RT2_ERR_INVALID, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    const hipError_t e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
    if (e != hipSuccess) return HipFail(e, call);
    return RT2_OK;
  }
};

// The chain's scratch, grown to `need` bytes.
static int EnsureScratch(const Chain& c, size_t need) {
  if (need > c.recon.d_scratch.bytes()) {
    HIP_TRY(c.recon.d_scratch.Grow(need));
    NoteDeviceBytes(c.t);
  }
  return RT2_OK;
}

// The chain's inputs at the head of its scratch, as the filter takes them: colour float3, then the variance of
// the mean. Enqueued on the tracer's stream.
static hipError_t EnqueueInputs(const Chain& c) {
  const size_t n = c.n();
  float* d_color = c.head();
  if (c.accum) return LaunchDenoiseInputs(c.accum, c.moment2, c.counts, d_color, (uint32_t)n, c.frames, c.t->stream);
  hipError_t e = hipMemcpyAsync(d_color, c.color, n * 3 * sizeof(float), hipMemcpyDeviceToDevice, c.t->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(d_color + 3 * n, c.variance, n * sizeof(float), hipMemcpyDeviceToDevice, c.t->stream);
  return e;
}

// The blend's kernels, enqueued on the chain's stream over a tracer that has passed its checks, with its frames
// launched (or its estimate gathered) and its features current; n > 0. The host does not wait. The blend of the
// current estimate with the history is left on the device: colour and variance at the head of the scratch (where
// LaunchDenoise takes them), the length in the chain's length plane; push: the result then replaces the history.
// scratch_bytes: what the scratch must hold at least. ev (or null): takes its two events from the pool and records
// them around the blend.
static int EnqueueBlend(const Chain& c, const TemporalParams& k, size_t scratch_bytes, bool push, EventPair* ev) {
  rt2_tracer* t = c.t;
  Recon& r = c.recon;
  const size_t n = c.n();
  int rc;
  HIP_TRY(hipSetDevice(t->device));
  if ((rc = EnsureScratch(c, scratch_bytes)) != RT2_OK) return rc;
  if (!r.d_hist) {
    r.tp_valid = false;
    HIP_TRY(r.d_hist.Alloc(TemporalHistoryBytes(n)));
    if (r.d_len.Alloc(n * sizeof(float)) != hipSuccess) {
      r.d_hist.reset();
      return Fail(RT2_ERR_HIP, "temporal: out of device memory");
    }
    NoteDeviceBytes(t);
  }
  float* d_color = c.head();
  if (ev && !ev->Take()) return Fail(RT2_ERR_HIP, "event create failed");
  hipError_t e = ev ? hipEventRecord(ev->e0, t->stream) : hipSuccess;
  if (e == hipSuccess) e = EnqueueInputs(c);
  if (e == hipSuccess)
    e = LaunchTemporalBlend(d_color, d_color + 3 * n, nullptr, c.counts, (float)c.frames, c.features(),
                            r.tp_valid ? r.d_hist.get<void>() : nullptr, r.tp_cam, t->d_materials.get<float>(),
                            t->n_materials, true, k, r.d_len.get<float>(), c.width, c.rows, t->stream);
  if (e == hipSuccess && ev) e = hipEventRecord(ev->e1, t->stream);
  if (e == hipSuccess && push) {
    r.tp_valid = false;  // until the pack has run
    e = LaunchTemporalPack(d_color, d_color + 3 * n, r.d_len.get<float>(), c.features(), r.d_hist.get<void>(), (uint32_t)n,
                           t->stream);
  }
  if (e != hipSuccess) return HipFail(e, "temporal");
  return RT2_OK;
}

static void CameraWords(const CameraParams& p, float* out) {  // rt2_camera_params' 21 words
  memcpy(out, p.pixel00, 3 * sizeof(float));
  memcpy(out + 3, p.du, 3 * sizeof(float));
  memcpy(out + 6, p.dv, 3 * sizeof(float));
  memcpy(out + 9, p.center, 3 * sizeof(float));
  memcpy(out + 12, p.defocus_u, 3 * sizeof(float));
  memcpy(out + 15, p.defocus_v, 3 * sizeof(float));
  out[18] = p.defocus_angle;
  out[19] = p.recip_sqrt_spp;
  out[20] = (float)p.sqrt_spp;
}

// After a pushing blend (EnqueueBlend, push): the history is held, under the camera it was rendered with.
static void HistoryPushed(const Chain& c) {
  CameraWords(c.t->camera.Params(), c.recon.tp_cam);
  c.recon.tp_valid = true;
}

// The chain's estimate blended into its history and kept as the history, before the camera moves on: blend and
// pack are enqueued on the tracer's stream, the host does not wait (n > 0, as EnqueueBlend).
static int PushHistory(const Chain& c, const TemporalParams& k) {
  int rc = EnqueueBlend(c, k, c.n() * 4 * sizeof(float), true, nullptr);
  if (rc == RT2_OK) HistoryPushed(c);
  return rc;
}

// The chain of rt2.h from the inputs to the copy into out_rgba, enqueued on the chain's stream over a tracer that
// has passed its checks, with its frames launched (or its estimate gathered) and its features current; n > 0.
// Nothing here blocks the host.
static int EnqueuePresent(const Chain& c, const PresentStages& st, uint8_t* out_rgba) {
  rt2_tracer* t = c.t;
  Recon& r = c.recon;
  const size_t n = c.n();
  int rc;
  HIP_TRY(hipSetDevice(t->device));
  // colour float3 and variance at the scratch's head, as the filter takes them; the RGBA8 words behind them, in
  // the filter's first plane, which is free again once the filter's last kernel (unpack) has run
  const size_t need = st.denoise ? DenoiseScratchBytes(n) : n * 5 * sizeof(float);
  if ((rc = EnsureScratch(c, need)) != RT2_OK) return rc;
  if ((rc = r.present_timer.Begin(t->stream)) != RT2_OK) return rc;
  if (st.temporal) {
    if ((rc = EnqueueBlend(c, st.tk, need, false, nullptr)) != RT2_OK) return rc;
  } else {
    HIP_TRY(EnqueueInputs(c));
  }
  float* d_color = c.head();
  uint8_t* d_rgba = reinterpret_cast<uint8_t*>(d_color + 4 * n);
  if (st.denoise) HIP_TRY(LaunchDenoise(d_color, c.features(), c.width, c.rows, st.dk, DenoiseLds(), t->stream));
  HIP_TRY(LaunchPresent(d_color, d_rgba, (uint32_t)n, t->stream));
  if ((rc = r.present_timer.End(t->stream)) != RT2_OK) return rc;
  HIP_TRY(hipMemcpyAsync(out_rgba, d_rgba, n * 4, hipMemcpyDeviceToHost, t->stream));
  return RT2_OK;
}

extern "C" {

// ---- feature buffers and denoiser (rt2.h "Feature buffers and denoiser") ----
void rt2_denoise_defaults(rt2_denoise_params* out) {
  if (!out) return;
  const DenoiseParams d = DenoiseDefaults();
  out->iterations = d.iterations;
  out->normal_power_log2 = d.normal_power_log2;
  out->sigma_l = d.sigma_l;
  out->sigma_p = d.sigma_p;
  out->sigma_a = d.sigma_a;
  out->eps_l = d.eps_l;
}

int rt2_tracer_features(rt2_tracer* t, float* out) {
  if (!t || !out) return Fail(RT2_ERR_INVALID, "null argument");
  if (IsMulti(t) || t->comm)
    return Fail(RT2_ERR_INVALID, "features: not on a multi-GPU or joined tracer (a set_partition tracer works)");
  int rc = FeaturesTimed(t);
  if (rc != RT2_OK) return rc;
  return ReadFeatures(t, t->recon, (size_t)t->width * (size_t)t->local_rows, out);
}

int rt2_tracer_denoise(rt2_tracer* t, const rt2_denoise_params* params, float* out_color, float* out_variance) {
  if (!t || !out_color) return Fail(RT2_ERR_INVALID, "null argument");
  if (!OneGpu(t)) return OneGpuRefusal("denoise");
  DenoiseParams k;
  int rc = DenoiseParamsOf(params, &k);
  if (rc != RT2_OK) return rc;
  if ((rc = LocalEstimateReady(t, "denoise")) != RT2_OK) return rc;
  const Chain c = LocalChain(t);
  const size_t n = c.n();
  if (n == 0) return RT2_OK;
  HIP_TRY(hipSetDevice(t->device));
  if ((rc = EnsureScratch(c, DenoiseScratchBytes(n))) != RT2_OK) return rc;
  EventPair ev(t);
  if (!ev.Take()) return Fail(RT2_ERR_HIP, "event create failed");
  hipError_t e = hipEventRecord(ev.e0, t->stream);
  if (e == hipSuccess) e = EnqueueInputs(c);
  if (e == hipSuccess) e = LaunchDenoise(c.head(), c.features(), c.width, c.rows, k, DenoiseLds(), t->stream);
  if (e == hipSuccess) e = hipEventRecord(ev.e1, t->stream);
  rc = ReadBack(e, c.head(), nullptr, n, out_color, out_variance, nullptr, t->stream, &t->host_waits, "denoise");
  if (rc != RT2_OK) return rc;
  t->denoise_ms = EventMs(ev);
  return RT2_OK;
}

int rt2_tracer_denoise_times(rt2_tracer* t, double* features_ms, double* denoise_ms) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  if (IsMulti(t)) return Fail(RT2_ERR_INVALID, "denoise_times: not on a multi-GPU tracer");
  if (features_ms) *features_ms = t->features_ms;
  if (denoise_ms) *denoise_ms = t->denoise_ms;
  return RT2_OK;
}

int rt2_denoise_buffers(int device, int width, int height, const float* color, const float* variance,
                        const float* features, const rt2_denoise_params* params, float* out_color, float* out_variance) {
  if (!color || !variance || !features || !out_color) return Fail(RT2_ERR_INVALID, "null argument");
  int rc = BufferCall::CheckSize("denoise_buffers", width, height);
  if (rc != RT2_OK) return rc;
  DenoiseParams k;
  if ((rc = DenoiseParamsOf(params, &k)) != RT2_OK) return rc;
  DeviceBuffer scratch, feat;  // (freed in the reverse order)
  BufferCall call;
  if ((rc = call.Open("denoise_buffers", device)) != RT2_OK) return rc;
  hipStream_t stream = call.stream;
  const size_t n = (size_t)width * (size_t)height;
  hipError_t e = scratch.Alloc(DenoiseScratchBytes(n));
  if (e == hipSuccess) e = feat.Alloc(n * kDenoiseFeatureFloats * sizeof(float));
  float* d_color = scratch.get<float>();
  float* d_feat = feat.get<float>();
  if (e == hipSuccess) e = hipMemcpyAsync(d_color, color, n * 3 * sizeof(float), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_color + 3 * n, variance, n * sizeof(float), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(d_feat, features, n * kDenoiseFeatureFloats * sizeof(float), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = LaunchDenoise(d_color, d_feat, width, height, k, DenoiseLds(), stream);
  return ReadBack(e, d_color, nullptr, n, out_color, out_variance, nullptr, stream, nullptr, "denoise_buffers");
}

// ---- temporal reuse (rt2.h "Temporal reuse") ----
void rt2_temporal_defaults(rt2_temporal_params* out) {
  if (!out) return;
  const TemporalParams d = TemporalDefaults();
  out->max_history = d.max_history;
  out->max_history_specular = d.max_history_specular;
  out->min_normal_dot = d.min_normal_dot;
  out->sigma_p = d.sigma_p;
  out->sigma_a = d.sigma_a;
}

// The blend of the tracer's current estimate with its history, left on the device (EnqueueBlend), after the checks
// of rt2_tracer_denoise.
static int TemporalBlend(rt2_tracer* t, const rt2_temporal_params* params, bool with_denoise, bool push, EventPair* ev) {
  if (!OneGpu(t)) return OneGpuRefusal("temporal");
  TemporalParams k;
  int rc = TemporalParamsOf(params, &k);
  if (rc != RT2_OK) return rc;
  if ((rc = LocalEstimateReady(t, "temporal")) != RT2_OK) return rc;
  const size_t n = (size_t)t->width * (size_t)t->local_rows;
  if (n == 0) return RT2_OK;
  return EnqueueBlend(LocalChain(t), k, with_denoise ? DenoiseScratchBytes(n) : n * 4 * sizeof(float), push, ev);
}

int rt2_tracer_temporal_resolve(rt2_tracer* t, const rt2_temporal_params* params, int denoise, const rt2_denoise_params* dparams,
                                float* out_color, float* out_variance, float* out_length) {
  if (!t || !out_color) return Fail(RT2_ERR_INVALID, "null argument");
  DenoiseParams dk = DenoiseDefaults();
  int rc = denoise ? DenoiseParamsOf(dparams, &dk) : RT2_OK;
  if (rc != RT2_OK) return rc;
  EventPair ev(t);
  if ((rc = TemporalBlend(t, params, denoise != 0, false, &ev)) != RT2_OK) return rc;
  const Chain c = LocalChain(t);
  const size_t n = c.n();
  if (n == 0) return RT2_OK;
  hipError_t e = hipSuccess;
  if (denoise) e = LaunchDenoise(c.head(), c.features(), c.width, c.rows, dk, DenoiseLds(), t->stream);
  rc = ReadBack(e, c.head(), c.recon.d_len.get<float>(), n, out_color, out_variance, out_length, t->stream, &t->host_waits,
                "temporal_resolve");
  if (rc != RT2_OK) return rc;
  t->temporal_ms = EventMs(ev);
  return RT2_OK;
}

int rt2_tracer_temporal_push(rt2_tracer* t, const rt2_temporal_params* params) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  int rc = TemporalBlend(t, params, false, true, nullptr);
  if (rc != RT2_OK) return rc;
  if ((size_t)t->width * (size_t)t->local_rows == 0) return RT2_OK;
  hipError_t e = hipStreamSynchronize(t->stream);
  t->host_waits++;
  if (e != hipSuccess) return HipFail(e, "temporal_push");
  HistoryPushed(LocalChain(t));
  return RT2_OK;
}

int rt2_tracer_temporal_clear(rt2_tracer* t) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  if (!OneGpu(t)) return OneGpuRefusal("temporal");
  t->recon.tp_valid = false;
  return RT2_OK;
}

int rt2_tracer_temporal_time(rt2_tracer* t, double* resolve_ms) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  if (IsMulti(t)) return Fail(RT2_ERR_INVALID, "temporal_time: not on a multi-GPU tracer");
  if (resolve_ms) *resolve_ms = t->temporal_ms;
  return RT2_OK;
}

int rt2_temporal_buffers(int device, int width, int height, const float* color, const float* variance, const float* length,
                         const float* features, const float* hist_color, const float* hist_variance,
                         const float* hist_length, const float* hist_features, const float* hist_camera,
                         const float* materials, int n_materials, const rt2_temporal_params* params, float* out_color,
                         float* out_variance, float* out_length) {
  if (!color || !variance || !length || !features || !hist_color || !hist_variance || !hist_length || !hist_features ||
      !hist_camera || !out_color)
    return Fail(RT2_ERR_INVALID, "null argument");
  int rc = BufferCall::CheckSize("temporal_buffers", width, height);
  if (rc != RT2_OK) return rc;
  if (n_materials < 0 || n_materials >= 1 << 24)
    return Fail(RT2_ERR_INVALID, "temporal_buffers: need 0 <= n_materials < 2^24");
  TemporalParams k;
  if ((rc = TemporalParamsOf(params, &k)) != RT2_OK) return rc;
  // cur / old: colour float3, variance, length; then the two feature images, the history planes, the table
  DeviceBuffer cur, old, feat, hfeat, out_len, hist, mat;  // (freed in the reverse order)
  BufferCall call;
  if ((rc = call.Open("temporal_buffers", device)) != RT2_OK) return rc;
  hipStream_t stream = call.stream;
  const size_t n = (size_t)width * (size_t)height;
  const size_t nf = n * kDenoiseFeatureFloats * sizeof(float);
  const bool mats = materials && n_materials > 0;
  hipError_t e = cur.Alloc(n * 5 * sizeof(float));
  if (e == hipSuccess) e = old.Alloc(n * 5 * sizeof(float));
  if (e == hipSuccess) e = feat.Alloc(nf);
  if (e == hipSuccess) e = hfeat.Alloc(nf);
  if (e == hipSuccess) e = out_len.Alloc(n * sizeof(float));
  if (e == hipSuccess) e = hist.Alloc(TemporalHistoryBytes(n));
  if (e == hipSuccess && mats) e = mat.Alloc((size_t)n_materials * kTemporalMaterialFloats * sizeof(float));
  float *d_cur = cur.get<float>(), *d_old = old.get<float>(), *d_feat = feat.get<float>(), *d_hfeat = hfeat.get<float>();
  float *d_out_len = out_len.get<float>(), *d_mat = mat.get<float>();
  void* d_hist = hist.get<void>();
  const auto up = [&](float* dst, const float* src, size_t bytes) {
    if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream);
  };
  up(d_cur, color, n * 3 * sizeof(float));
  up(d_cur + 3 * n, variance, n * sizeof(float));
  up(d_cur + 4 * n, length, n * sizeof(float));
  up(d_old, hist_color, n * 3 * sizeof(float));
  up(d_old + 3 * n, hist_variance, n * sizeof(float));
  up(d_old + 4 * n, hist_length, n * sizeof(float));
  up(d_feat, features, nf);
  up(d_hfeat, hist_features, nf);
  if (mats) up(d_mat, materials, (size_t)n_materials * kTemporalMaterialFloats * sizeof(float));
  if (e == hipSuccess) e = LaunchTemporalPack(d_old, d_old + 3 * n, d_old + 4 * n, d_hfeat, d_hist, (uint32_t)n, stream);
  if (e == hipSuccess)
    e = LaunchTemporalBlend(d_cur, d_cur + 3 * n, d_cur + 4 * n, nullptr, 0.0f, d_feat, d_hist, hist_camera, d_mat,
                            mats ? n_materials : 0, false, k, d_out_len, width, height, stream);
  return ReadBack(e, d_cur, d_out_len, n, out_color, out_variance, out_length, stream, nullptr, "temporal_buffers");
}

// ---- presenting reconstructed frames (rt2.h "Presenting reconstructed frames") ----
void rt2_present_defaults(rt2_present_params* out) {
  if (!out) return;
  out->temporal = 1;
  out->denoise = 1;
  rt2_temporal_defaults(&out->tp);
  rt2_denoise_defaults(&out->dp);
}

// The chain of rt2.h, enqueued on the tracer's stream; every refusal comes before the first enqueue. Nothing
// here blocks the host: no stream or event synchronisation, no synchronous copy (growing a buffer at the first
// call is the exception every first call has).
int rt2_tracer_present_async(rt2_tracer* t, const rt2_present_params* params, uint8_t* out_rgba) {
  if (!t || !out_rgba) return Fail(RT2_ERR_INVALID, "null argument");
  if (!OneGpu(t)) return OneGpuRefusal("present");
  PresentStages st;
  int rc = PresentStagesOf(params, &st);
  if (rc != RT2_OK) return rc;
  if (!t->moments_on) return MomentsRefusal("present");
  if (t->frame_idx + t->queued < 2) return FramesRefusal("present");
  if ((rc = Flush(t)) != RT2_OK) return rc;
  if ((rc = LocalFeatures(t, nullptr, nullptr)) != RT2_OK) return rc;
  const Chain c = LocalChain(t);
  if (c.n() == 0) return RT2_OK;
  return EnqueuePresent(c, st, out_rgba);
}

int rt2_tracer_present(rt2_tracer* t, const rt2_present_params* params, uint8_t* out_rgba) {
  int rc = rt2_tracer_present_async(t, params, out_rgba);
  return rc != RT2_OK ? rc : Sync(t);
}

int rt2_tracer_move_camera(rt2_tracer* t, const rt2_camera_desc* cam, const rt2_temporal_params* params) {
  if (!t || !cam) return Fail(RT2_ERR_INVALID, "null argument");
  if (IsMulti(t) || t->comm) return Fail(RT2_ERR_INVALID, "move_camera: not on a multi-GPU or joined tracer");
  TemporalParams k;
  int rc = TemporalParamsOf(params, &k);
  if (rc != RT2_OK) return rc;
  const size_t n = (size_t)t->width * (size_t)t->local_rows;
  if (t->world == 1 && t->moments_on && t->frame_idx + t->queued >= 2 && n > 0) {
    // the push of rt2_tracer_temporal_push without its wait: blend and pack are on the tracer's stream, and so
    // is every memset of ResetFrame below, so the sums are zeroed after the pack's inputs kernel has read them
    if ((rc = Flush(t)) != RT2_OK) return rc;
    if ((rc = LocalFeatures(t, nullptr, nullptr)) != RT2_OK) return rc;
    if ((rc = PushHistory(LocalChain(t), k)) != RT2_OK) return rc;
  }
  if ((rc = rt2_tracer_set_camera(t, cam)) != RT2_OK) return rc;
  return rt2_tracer_reset(t);
}

int rt2_tracer_present_time(rt2_tracer* t, double* ms) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  if (!OneGpu(t)) return OneGpuRefusal("present");
  return t->recon.present_timer.Poll(t->device, "present_time", ms);  // polls, never waits
}

int rt2_present_buffers(int device, int width, int height, const float* color, uint8_t* out_rgba) {
  if (!color || !out_rgba) return Fail(RT2_ERR_INVALID, "null argument");
  int rc = BufferCall::CheckSize("present_buffers", width, height);
  if (rc != RT2_OK) return rc;
  DeviceBuffer col, px;  // (freed in the reverse order)
  BufferCall call;
  if ((rc = call.Open("present_buffers", device)) != RT2_OK) return rc;
  hipStream_t stream = call.stream;
  const size_t n = (size_t)width * (size_t)height;
  hipError_t e = col.Alloc(n * 3 * sizeof(float));
  if (e == hipSuccess) e = px.Alloc(n * 4);
  if (e == hipSuccess) e = hipMemcpyAsync(col.get<float>(), color, n * 3 * sizeof(float), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = LaunchPresent(col.get<float>(), px.get<void>(), (uint32_t)n, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out_rgba, px.get<uint8_t>(), n * 4, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return HipFail(e, "present_buffers");
  return RT2_OK;
}

// ---- reconstructing the gathered image (rt2.h "Reconstructing the gathered image") ----
static const char kImageRankMsg[] = "the gathered image lives on rank 0";

// The root of the gathered image, with the estimate of the current FrameIdx() and the whole-image features
// enqueued on its stream. Every refusal comes before the first enqueue.
static int ImageReady(rt2_tracer* t, rt2_tracer** root) {
  const rt2_tracer* first = IsMulti(t) ? t->parts[0] : t;
  if (first->rank != 0) return Fail(RT2_ERR_INVALID, kImageRankMsg);
  if (!first->stack_ok) return StackRefusal(first);
  int rc = CurrentEstimate(t, false, root);
  if (rc != RT2_OK) return rc;
  return ImageFeatures(*root);
}

int rt2_tracer_image_features(rt2_tracer* t, float* out) {
  if (!t || !out) return Fail(RT2_ERR_INVALID, "null argument");
  rt2_tracer* r = IsMulti(t) ? t->parts[0] : t;
  if (r->rank != 0) return Fail(RT2_ERR_INVALID, kImageRankMsg);
  int rc = ImageFeatures(r);
  if (rc != RT2_OK) return rc;
  return ReadFeatures(r, r->image_recon, (size_t)r->width * (size_t)r->height, out);
}

int rt2_tracer_image_resolve(rt2_tracer* t, const rt2_present_params* params, float* out_color, float* out_variance,
                             float* out_length) {
  if (!t || !out_color) return Fail(RT2_ERR_INVALID, "null argument");
  PresentStages st;
  int rc = PresentStagesOf(params, &st);
  if (rc != RT2_OK) return rc;
  rt2_tracer* r = nullptr;
  if ((rc = ImageReady(t, &r)) != RT2_OK) return rc;
  const Chain c = ImageChain(r);
  const size_t n = c.n();
  if (n == 0) return RT2_OK;
  const size_t need = st.denoise ? DenoiseScratchBytes(n) : n * 4 * sizeof(float);
  if (st.temporal) {
    if ((rc = EnqueueBlend(c, st.tk, need, false, nullptr)) != RT2_OK) return rc;
  } else {
    HIP_TRY(hipSetDevice(r->device));
    if ((rc = EnsureScratch(c, need)) != RT2_OK) return rc;
    HIP_TRY(EnqueueInputs(c));
  }
  hipError_t e = hipSuccess;
  if (st.denoise) e = LaunchDenoise(c.head(), c.features(), c.width, c.rows, st.dk, DenoiseLds(), r->stream);
  // the length plane is the blend's: with the temporal stage off it is not copied (out_length is left untouched)
  return ReadBack(e, c.head(), c.recon.d_len.get<float>(), n, out_color, out_variance, st.temporal ? out_length : nullptr,
                  r->stream, &r->host_waits, "image_resolve");
}

int rt2_tracer_image_present_async(rt2_tracer* t, const rt2_present_params* params, uint8_t* out_rgba) {
  if (!t || !out_rgba) return Fail(RT2_ERR_INVALID, "null argument");
  PresentStages st;
  int rc = PresentStagesOf(params, &st);
  if (rc != RT2_OK) return rc;
  rt2_tracer* r = nullptr;
  if ((rc = ImageReady(t, &r)) != RT2_OK) return rc;
  const Chain c = ImageChain(r);
  if (c.n() == 0) return RT2_OK;
  return EnqueuePresent(c, st, out_rgba);
}

int rt2_tracer_image_present(rt2_tracer* t, const rt2_present_params* params, uint8_t* out_rgba) {
  int rc = rt2_tracer_image_present_async(t, params, out_rgba);
  return rc != RT2_OK ? rc : rt2_tracer_synchronize(t);
}

int rt2_tracer_image_move_camera(rt2_tracer* t, const rt2_camera_desc* cam, const rt2_temporal_params* params) {
  if (!t || !cam) return Fail(RT2_ERR_INVALID, "null argument");
  TemporalParams k;
  int rc = TemporalParamsOf(params, &k);
  if (rc != RT2_OK) return rc;
  const rt2_tracer* first = IsMulti(t) ? t->parts[0] : t;
  if (!IsMulti(t) && !t->comm && t->world > 1)
    return Fail(RT2_ERR_INVALID, "image_move_camera: a partitioned tracer must be joined to a communicator");
  if (first->adaptive_on && !first->image_adaptive)
    return Fail(RT2_ERR_INVALID, "image_move_camera: adaptive sampling is on (rt2_tracer_move_camera keeps its history)");
  const size_t n = (size_t)first->width * (size_t)first->height;
  if (first->moments_on && first->frame_idx + first->queued >= 2 && n > 0) {
    if (!first->stack_ok) return StackRefusal(first);
    // the estimate's kernel, the blend and the pack run on the root's stream and read only the root's gathered
    // buffers; the parts' sums were read by the gather, which every part's stream is ordered behind (its own
    // ncclGather, or the event after the root's copies), so the memsets of the reset below come after it
    rt2_tracer* r = nullptr;
    if ((rc = CurrentEstimate(t, true, &r)) != RT2_OK) return rc;
    if (r->rank == 0) {
      if ((rc = ImageFeatures(r)) != RT2_OK) return rc;
      if ((rc = PushHistory(ImageChain(r), k)) != RT2_OK) return rc;
    }
  }
  if ((rc = rt2_tracer_set_camera(t, cam)) != RT2_OK) return rc;
  return rt2_tracer_reset(t);
}

int rt2_tracer_image_present_time(rt2_tracer* t, double* ms) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  rt2_tracer* r = IsMulti(t) ? t->parts[0] : t;
  if (r->rank != 0) return Fail(RT2_ERR_INVALID, kImageRankMsg);
  return r->image_recon.present_timer.Poll(r->device, "present_time", ms);
}
}  // extern "C"
