// tracer.h — what the capi*.cpp files share (internal): the handles behind include/rt2.h, the buffer types
// that own the tracer's device memory, the error helpers, and the helpers that cross those files.
#pragma once

#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rt2.h"
#include "kernels.h"
#include "scene.h"

namespace rt2 {

// Device memory from hipMalloc, freed with hipFree. Move-only; bytes() is what it holds (the tracer's
// device-byte accounting sums these).
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(DeviceBuffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      bytes_ = std::exchange(o.bytes_, 0);
    }
    return *this;
  }
  ~DeviceBuffer() { reset(); }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    bytes_ = 0;
  }
  hipError_t Alloc(size_t bytes) {  // frees what it holds first
    reset();
    const hipError_t e = hipMalloc(&p_, bytes);
    if (e != hipSuccess) p_ = nullptr;
    else bytes_ = bytes;
    return e;
  }
  hipError_t Grow(size_t bytes) { return bytes > bytes_ ? Alloc(bytes) : hipSuccess; }  // never shrinks
  hipError_t Upload(const void* src, size_t bytes) {
    const hipError_t e = Alloc(bytes);
    return e != hipSuccess ? e : hipMemcpy(p_, src, bytes, hipMemcpyHostToDevice);
  }
  template <typename T>
  T* get() const {
    return static_cast<T*>(p_);
  }
  size_t bytes() const { return bytes_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  void* p_ = nullptr;
  size_t bytes_ = 0;
};

// Device memory from hipMallocAsync, freed with hipFreeAsync on the stream it was allocated on: the queued
// work that still uses the old memory runs first, and the host does not wait (hipFree would synchronize the
// device; a multi-GPU tracer enqueues every GPU's render before any of them finishes).
class StreamBuffer {
 public:
  StreamBuffer() = default;
  StreamBuffer(StreamBuffer&& o) noexcept
      : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)), stream_(o.stream_) {}
  StreamBuffer& operator=(StreamBuffer&& o) noexcept {
    if (this != &o) {
      (void)reset();
      p_ = std::exchange(o.p_, nullptr);
      bytes_ = std::exchange(o.bytes_, 0);
      stream_ = o.stream_;
    }
    return *this;
  }
  ~StreamBuffer() { (void)reset(); }
  hipError_t reset() {
    const hipError_t e = p_ ? hipFreeAsync(p_, stream_) : hipSuccess;
    p_ = nullptr;
    bytes_ = 0;
    return e;
  }
  hipError_t Alloc(size_t bytes, hipStream_t stream) {  // frees what it holds first (on its own stream)
    hipError_t e = reset();
    if (e != hipSuccess) return e;
    stream_ = stream;
    e = hipMallocAsync(&p_, bytes, stream);
    if (e != hipSuccess) p_ = nullptr;
    else bytes_ = bytes;
    return e;
  }
  template <typename T>
  T* get() const {
    return static_cast<T*>(p_);
  }
  size_t bytes() const { return bytes_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  void* p_ = nullptr;
  size_t bytes_ = 0;
  hipStream_t stream_ = nullptr;
};

}  // namespace rt2

// Default bound on the per-frame sample buffers of both launch slots together (rt2.h
// rt2_tracer_set_sample_budget). Each slot gets half, so a 1024^2 image runs 1000 frames (11.7 GiB of
// samples) in one launch per slot: the headline renders one launch per step. Measured on the final
// round-6 kernel, one MI355X: DESIGN.md §3 "Sample buffer budget".
constexpr size_t kDefaultSampleBudget = size_t(24) << 30;

struct rt2_scene {
  rt2::Scene scene;
  rt2::CompiledScene compiled;
};

namespace rt2::detail {

int Fail(int code, const std::string& m);  // sets rt2_last_error's text (one thread_local, capi.cpp)
int HipFail(hipError_t e, const char* what);
#define HIP_TRY(expr)                                  \
  do {                                                 \
    hipError_t _e = (expr);                            \
    if (_e != hipSuccess) return HipFail(_e, #expr);   \
  } while (0)

#define NCCL_TRY(expr)                                                                     \
  do {                                                                                     \
    ncclResult_t _r = (expr);                                                              \
    if (_r != ncclSuccess) return Fail(RT2_ERR_HIP, std::string(#expr) + ": " + ncclGetErrorString(_r)); \
  } while (0)

// The GPU time of one family's last call (-1: none): two events (created at the first device entry, re-recorded by
// every later one), whether that call's time is still to be read from them, and the last time read. A device entry
// brackets its kernels with Begin and End and does not wait; a host entry, which has waited, Sets the sum it
// measured; the family's _time export Polls. Release is ~rt2_tracer's, at the events' place in its order (no
// destructor: it would call HIP at a time nobody chose).
struct KernelTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  bool pending = false;
  double ms = -1.0;

  int Begin(hipStream_t stream) {
    if (!e0 && hipEventCreate(&e0) != hipSuccess) return Fail(RT2_ERR_HIP, "event create failed");
    if (!e1 && hipEventCreate(&e1) != hipSuccess) return Fail(RT2_ERR_HIP, "event create failed");
    pending = false;
    ms = -1.0;
    HIP_TRY(hipEventRecord(e0, stream));
    return RT2_OK;
  }
  int End(hipStream_t stream) {
    HIP_TRY(hipEventRecord(e1, stream));
    pending = true;
    return RT2_OK;
  }
  void Set(double measured_ms) {
    pending = false;
    ms = measured_ms;
  }
  // *out (or null): -1 while the call is pending, else the time, which is read from the events once and kept. Never
  // waits; `what` names the export in the report of anything but not-ready.
  int Poll(int device, const char* what, double* out) {
    if (pending) {
      HIP_TRY(hipSetDevice(device));
      const hipError_t q = hipEventQuery(e1);
      if (q == hipSuccess) {
        float f = -1.0f;
        if (hipEventElapsedTime(&f, e0, e1) != hipSuccess) f = -1.0f;
        ms = (double)f;
        pending = false;
      } else if (q != hipErrorNotReady) {
        return HipFail(q, what);
      }
    }
    if (out) *out = pending ? -1.0 : ms;
    return RT2_OK;
  }
  void Release() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    e0 = e1 = nullptr;
  }
};

// The reconstruction state of one image: a one-GPU tracer's local rows, or the gathered image on its root (the
// tracer holds one of each; capi_filter.cpp runs the same chain over either). Every buffer is allocated at the
// first call that needs it. The cached feature records (rt2.h "Feature buffers and denoiser") with the launch
// values they were traced under; the filter's scratch planes, whose head holds the chain's colour and variance;
// temporal reuse (rt2.h "Temporal reuse"): the packed history (temporal.hip's four planes) and the blend's length
// plane, whether a history is held and the camera words it was pushed under; presenting (rt2.h "Presenting
// reconstructed frames"): the timer of the last present's kernels (rt2_tracer_present_time polls it).
struct Recon {
  DeviceBuffer d_features;  // 16 floats per pixel
  bool features_valid = false;
  CameraParams features_cam;
  uint64_t features_seed = 0;
  DeviceBuffer d_scratch;
  DeviceBuffer d_hist;
  DeviceBuffer d_len;
  bool tp_valid = false;
  float tp_cam[kTemporalCameraWords] = {};
  KernelTimer present_timer;

  // Its device buffers, listed once, in the order they are freed. R: Recon or const Recon.
  template <typename R, typename Fn>
  static void ForBuffers(R& r, Fn&& f) {
    for (auto* d : {&r.d_features, &r.d_scratch, &r.d_hist, &r.d_len}) f(*d);
  }
  // Drops the buffers, and the records and the history with them (a resize); the present timer stays.
  void Free() {
    ForBuffers(*this, [](DeviceBuffer& d) { d.reset(); });
    features_valid = false;
    tp_valid = false;
  }
  size_t Bytes() const {
    size_t b = 0;
    ForBuffers(*this, [&b](const DeviceBuffer& d) { b += d.bytes(); });
    return b;
  }
};

}  // namespace rt2::detail

struct rt2_tracer {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  // scene program
  rt2::DeviceBuffer d_nodes;
  rt2::DeviceBuffer d_materials;
  rt2::DeviceBuffer d_textures;
  rt2::DeviceBuffer d_perlin_vec;
  rt2::DeviceBuffer d_perlin_perm;
  rt2::DeviceBuffer d_lin;
  rt2::DeviceBuffer d_lin_wide;
  rt2::DeviceBuffer d_lind;
  rt2::DeviceBuffer d_hit;        // hit table (rt2_layout.h HIT); null: the scene has none
  int hit_key = -1;             // cached: the kernel variant asked whether the table keeps its occupancy
  bool hit_fits = false;
  uint32_t last_hit_bytes = 0;  // the table the last launch staged in LDS (0: none)
  // flat program (rt2_layout.h "Flat program"): its wide steps, the certificate table, the FlatMode; null / 0:
  // the scene has none
  rt2::DeviceBuffer d_flat_wide;
  rt2::DeviceBuffer d_flat_cert;
  uint32_t flat_mode = 0;
  uint32_t lin_len = 0;
  bool use_linear = true;
  uint32_t root = rt2::kRefNone;
  uint32_t node_records = 0;
  uint32_t features = 0;
  int max_stack = 1;
  bool stack_ok = true;  // the scene fits the stack traversal (else only the threaded program runs it)
  bool flat_xforms = true;  // no nested transforms in the threaded program (RenderParams::flat_xforms)
  bool origins_bounded = false;  // CompiledScene::origins_bounded: launches check the camera's range
  bool use_lds = true;
  bool use_hybrid = true;   // stage only the BVH prefix in LDS when the scene is too large
  bool force_hybrid = false;  // tests: hybrid even when the whole scene would fit
  uint32_t hot_records = 0;
  int cus = 0;
  int lds_per_cu = 0;       // bytes of LDS per CU
  int hybrid_cap = -1;      // tests: most BVH records staged by the hybrid mode (-1: no cap)
  int hyb_key = -1;         // cached hybrid prefix for (variant, counting)
  uint32_t hyb_records = 0;
  float background[3] = {0, 0, 0};
  rt2::Camera camera;  // RayTracer::camera (a copy of the scene camera)
  // frame buffers (local rows)
  int width = 0, height = 0, local_rows = 0;
  int band_h = 0, rank = 0, world = 1;
  rt2::DeviceBuffer d_accum;
  rt2::DeviceBuffer d_pixels;
  rt2::DeviceBuffer d_ray_counts;
  bool ray_counts_on = false;
  // moments (rt2_tracer_enable_moments): float3 sums of the samples' squares per local pixel, summed in
  // frame order by the accumulate pass; d_noise holds the noise kernel's per-workgroup partials
  rt2::DeviceBuffer d_moment2;
  bool moments_on = false;
  rt2::DeviceBuffer d_noise;
  // adaptive sampling (rt2_tracer_enable_adaptive; needs moments): per local pixel its sample count n_p
  // and active flag, the check's `over` flags, the list of the active pixels (tile-major, padded to 64:
  // adaptive.hip) and each pixel's slot in it, and the check's per-workgroup scratch. n_active is what
  // the last check left (all local pixels after a reset); launches take the list once a pixel has retired.
  bool adaptive_on = false;
  // adaptive sampling of the gathered image (rt2_tracer_image_enable_adaptive): adaptive_on, and the counts travel
  // with the gather. The refusals of the gathered-image calls key on adaptive_on && !image_adaptive.
  bool image_adaptive = false;
  rt2::DeviceBuffer d_counts;
  rt2::DeviceBuffer d_active;
  rt2::DeviceBuffer d_over;
  rt2::DeviceBuffer d_list;
  rt2::DeviceBuffer d_slot_of;
  rt2::DeviceBuffer d_ad_scratch;  // wg counts (uint2), wg offsets, classify partials, totals
  uint32_t n_active = 0;
  // what the last check left of this tracer's own pixels (rt2_tracer_image_part_adaptive; frames 0: none since the
  // last reset), and the image check's pinned host words and, on a joined tracer, the device words its all-reduce
  // sums in place (capi_estimate.cpp ImageCheck; allocated at the first image check)
  rt2_adaptive last_check = {};
  unsigned long long* h_check = nullptr;
  rt2::DeviceBuffer d_check_sum;
  // the reconstruction of the local rows (Recon above) and the GPU times of the last feature pass, the last
  // denoise and the last resolve's temporal kernels (-1: none), which only the local calls report
  rt2::detail::Recon recon;
  double features_ms = -1.0, denoise_ms = -1.0, temporal_ms = -1.0;
  int n_materials = 0;  // materials in d_materials
  // ray queries (rt2.h "Ray queries", capi_query.cpp): the host entries' two device buffers (rays in, records out),
  // grown on demand and kept, which every family's chunks go through (ChunkedHostCall); and one timer per family,
  // each of its own calls alone: intersect's and occluded's (rt2_tracer_intersect_time), ambient occlusion's
  // (rt2_tracer_ambient_time), the radiance queries' (rt2_tracer_radiance_time)
  rt2::DeviceBuffer d_query_rays;
  rt2::DeviceBuffer d_query_hits;
  rt2::detail::KernelTimer query_timer, ambient_timer, radiance_timer;
  // radiance queries: the result slots of a launch's (ray, sample) items, grown on demand and kept
  rt2::DeviceBuffer d_radiance_slots;
  rt2::DeviceBuffer d_work;  // one work counter per launch slot (words 0 and 16)
  rt2::DeviceBuffer d_stats;
  bool stats_on = false;
  int64_t frame_idx = 0;  // frames launched (FrameIdx() = frame_idx + queued)
  int queued = 0;         // Update()/Render() frames not launched yet (lazy, see rt2_tracer_render)
  int lazy_max = 4096;    // launch once this many frames are queued (0: launch at every call)
  int max_depth = 50;
  uint64_t seed = 0x5EED2024ull;
  int launch_frames = 0;
  // Launch slots: a render launch runs on one of two render streams with that slot's per-frame
  // sample buffer ([frames][local pixels] float3, which lets a pixel's frames be split into chunks
  // rendered by different lanes and still be summed in frame order), chunk table and work counter;
  // its accumulate_kernel runs on the tracer's stream after it. Consecutive launches alternate
  // slots, so a launch does not wait for the previous one: its waves take the CUs the previous
  // launch's tail leaves idle (LaunchFrames).
  struct Slot {
    hipStream_t stream = nullptr;
    rt2::StreamBuffer samples;
    rt2::StreamBuffer chunks;           // this slot's chunk table (ChunkSchedule)
    std::vector<uint32_t> chunks_host;  // what `chunks` holds (renders repeat one schedule: no upload)
    hipEvent_t rendered = nullptr;      // the slot's last render launch finished (tracer stream waits)
    hipEvent_t consumed = nullptr;      // the accumulate that last read `samples` finished
    bool consumed_set = false;
  };
  Slot slots[2];
  int next_slot = 0;
  bool pipeline = true;  // RT2_PIPELINE=0: every launch waits for the tracer stream (no overlap)
  // bytes: the bound on both launch slots' sample buffers together (each slot gets half; a render
  // needing more runs as several launches, rt2.h rt2_tracer_set_sample_budget)
  size_t sample_budget = kDefaultSampleBudget;
  size_t device_bytes_peak = 0;   // high-water mark of DeviceBytes()
  // chunk schedule: work left split into >= k items per lane (0: one chunk). 4 since round 6: a launch with
  // few pixels per lane (an 8-way rank) gets 60-frame chunks instead of 12 (emulated 8-way C2 job +4.8 %);
  // full-size launches are capped at 64-frame chunks either way
  int work_split = 4;
  int chunk_max = 64;                      // longest chunk (frames)
  int frame_tiles_env = -1;                // RT2_FRAME_TILES: -1 auto, 0 off, 1 on
  bool frame_tiles = false;                // this launch: items = one pixel x 64 short chunks per wave
  int frame_tile_len = 8;                  // most frames per chunk in frame-tile mode (RT2_FRAME_TILE_LEN)
  bool chunk_align = true;                 // chunks of >= kOctet frames: multiples of 4 frames
  struct Staging {                         // pinned host copies of uploaded tables, reusable once copied
    uint32_t* p;
    size_t bytes;
    hipEvent_t done;
  };
  std::vector<Staging> staging;
  int batch_max = 64;                      // most work items a wave reserves with one atomic
  int last_chunk_frames = 0;
  int occ_key = -1, occ_blocks = 1;  // cached occupancy of the last kernel instantiation
  size_t occ_lds = 0;
  int last_variant = -1;
  int last_grid = 0;
  uint64_t launches = 0;
  uint64_t paths = 0;
  // Render-kernel time, from the launches' own clocks (RenderParams::launch_clock): a ring of
  // kClockRing (start complement, end) pairs on the device, read back at the next synchronization.
  // kernel_ms is the time at least one render launch of this tracer ran (the union of the launches'
  // first-wave-to-last-wave intervals: consecutive launches overlap in a launch's tail);
  // launch_ms_sum adds the intervals up (the overlap counted twice).
  double kernel_ms = 0;
  double launch_ms_sum = 0;
  rt2::DeviceBuffer d_clock;  // [kClockRing][2]
  unsigned long long* h_clock = nullptr;  // pinned copy
  uint32_t clock_next = 0;                // next ring entry
  std::vector<uint32_t> pending;          // ring entries of launches not yet read back
  double clock_khz = 100000.0;            // hipDeviceAttributeWallClockRate
  unsigned long long busy_end = 0;        // end of the union so far (clock ticks)
  std::vector<hipEvent_t> event_pool;
  // ---- multi-GPU ----
  std::vector<rt2_tracer*> parts;  // multi tracer: one one-GPU tracer per device, parts[i] = rank i
  bool loopback = false;           // the parts share one GPU: device-local copies instead of RCCL
  ncclComm_t comm = nullptr;       // this tracer's rank in an RCCL communicator (a part, or joined)
  // root (rank 0) image: the gathered band stacks and the de-interleaved full image
  rt2::DeviceBuffer d_stacks;      // [world][max_rows][W] float3
  rt2::DeviceBuffer d_image;       // [H][W] float3
  rt2::DeviceBuffer d_image_nc;    // [H][W] float3 NonConvertedPixels() = image / frame_idx
  rt2::DeviceBuffer d_image_px;    // [H][W] RGBA8
  int64_t image_frame = -1;  // frame index of the last gather (-1: none since the last resize/reset)
  uint64_t gathers = 0;
  double gather_ms = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> gpending;  // per-gather timing events
  // root: the gathered stacks of the sums of squares and the variance of the mean in image order
  // (rt2_tracer_gather_estimate), allocated at the first call, with the frame index they are of (-1: none); and
  // the reconstruction of the gathered image (rt2.h "Reconstructing the gathered image")
  rt2::DeviceBuffer d_stacks2;       // [world][max_rows][W] float3
  rt2::DeviceBuffer d_image_var;     // [H][W] float
  int64_t estimate_frame = -1;
  // root, with image_adaptive on: the gathered stacks of the sample counts and n_p in image order, allocated at the
  // first gather that carries them; image_counts: the last gather wrote them (the chain's lengths are then n_p)
  rt2::DeviceBuffer d_stacks_n;      // [world][max_rows][W] uint32
  rt2::DeviceBuffer d_image_n;       // [H][W] uint32
  bool image_counts = false;
  rt2::detail::Recon image_recon;
  // image readbacks to the host (rt2_tracer_image_*): count and device-to-host copy time
  uint64_t readbacks = 0;
  double readback_ms = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> rpending;  // async readbacks' timing events
  double enqueue_ms = 0;  // host time spent enqueueing this tracer's renders (LaunchFrames)
  uint64_t host_waits = 0;  // times the library blocked the host on this GPU (stream / event syncs, sync copies)
  rt2_tracer() = default;
  rt2_tracer(const rt2_tracer&) = delete;
  rt2_tracer& operator=(const rt2_tracer&) = delete;
  ~rt2_tracer();  // capi.cpp: releases everything the tracer holds on its GPU, in an explicit order
};

namespace rt2::detail {

// capi.cpp
int LocalRows(int h, int band_h, int rank, int world);
void FreeImage(rt2_tracer* t);
void NoteDeviceBytes(rt2_tracer* t);
int Realloc(rt2_tracer* t);
int ResetFrame(rt2_tracer* t);
hipEvent_t TakeEvent(rt2_tracer* t);
int Flush(rt2_tracer* t);  // launches the queued frames (rt2_tracer_render)
int Sync(rt2_tracer* t);
// The RenderParams every kernel over the scene takes: the scene tables and root, background, camera, image
// and partition, seed and Philox keys, stack depth; everything else zero.
void BaseParams(const rt2_tracer* t, const CameraParams& cam, RenderParams* p);
// capi_estimate.cpp: the two halves of an adaptive check over the tracer's local pixels, whose frames are launched
// and number at least 2. Enqueue: the check's kernels on the tracer's stream and, with `host` not null, the copy
// of their totals into it; d_totals (or null) receives where the totals lie on the device. Nothing is enqueued for
// a tracer without a pixel (*host zeroed). Finish, after the stream has been waited for: the local totals become
// the tracer's n_active and last_check, and *out (or null).
int EnqueueAdaptiveCheck(rt2_tracer* t, float threshold, int window, rt2::AdaptiveTotals* host,
                         rt2::AdaptiveTotals** d_totals);
int FinishAdaptiveCheck(rt2_tracer* t, const rt2::AdaptiveTotals& h, rt2_adaptive* out);
int SampleCountsLocal(rt2_tracer* t, uint32_t* out);  // n_p per local pixel of an adaptive one-GPU tracer (blocks)
// capi_filter.cpp: the cached feature records of a one-GPU tracer's local rows as traced under `seed` (the cache
// is keyed by camera, size, partition and seed), traced again on the tracer's stream where stale; no host wait.
int FeaturesForSeed(rt2_tracer* t, uint64_t seed, const float** d_features);
// capi_multi.cpp
int GatherMulti(rt2_tracer* t);
int GatherEstimate(rt2_tracer* t);  // rt2_tracer_gather_estimate: the gather with the sums of squares
// The tracer holding the gathered image (rank 0) with the estimate of the current FrameIdx() (queued frames
// included) enqueued on it. A create_multi or plain tracer whose estimate is missing or stale gathers here; a
// joined one is refused, unless `collective`: then every rank is calling, a rank that is behind takes part in the
// gather, and a rank other than 0 gets itself back (it holds no image).
int CurrentEstimate(rt2_tracer* t, bool collective, rt2_tracer** root);

inline int BandH(const rt2_tracer* t) { return t->band_h > 0 ? t->band_h : (t->height > 0 ? t->height : 1); }

// Rows of the largest rank's band stack (every rank's accumulation is allocated this tall, so the
// gather sends equal counts; the padding rows stay zero).
inline int BandRowsMax(const rt2_tracer* t) { return rt2::BandRowsMax(t->height, t->band_h, t->world); }

// Rows of the accumulation buffer: the gather sends BandRowsMax rows from every rank, also at world 1
// (a band height that does not divide the image height leaves padding rows), so every buffer is that
// tall; the rows past local_rows stay zero.
inline int AllocRows(const rt2_tracer* t) { return BandRowsMax(t); }

inline bool IsMulti(const rt2_tracer* t) { return !t->parts.empty(); }

// Applies f to every part of a multi tracer (stops at the first error).
template <typename Fn>
int ForParts(rt2_tracer* t, Fn&& f) {
  for (rt2_tracer* p : t->parts) {
    int rc = f(p);
    if (rc != RT2_OK) return rc;
  }
  return RT2_OK;
}

// Forwards a setter to every part of a multi tracer.
#define RT2_FORWARD(t, call)                                           \
  do {                                                                 \
    if (IsMulti(t)) return ForParts(t, [&](rt2_tracer* p) { return call; }); \
  } while (0)

// A per-pixel readback of a multi tracer that needs no gather (diagnostics): read(part, rows) fills each
// GPU's local rows (`ch` values of T per pixel), which are placed in image order on the host.
template <typename T, typename Fn>
int PlacePartRows(rt2_tracer* t, T* out, int ch, Fn&& read) {
  std::vector<T> part;
  for (rt2_tracer* p : t->parts) {
    const size_t row = (size_t)p->width * (size_t)ch;
    part.resize(row * (size_t)p->local_rows);
    int rc = read(p, part.data());
    if (rc != RT2_OK) return rc;
    const int bh = BandH(p);
    for (int r = 0; r < p->local_rows; r++) {
      const int period = r / bh;  // the rank's band of this period (rt2_layout.h BandRank)
      const int phase = ((p->rank - period) % p->world + p->world) % p->world;
      const int y = (period * p->world + phase) * bh + r % bh;
      memcpy(out + (size_t)y * row, part.data() + (size_t)r * row, row * sizeof(T));
    }
  }
  return RT2_OK;
}

// Two events borrowed from the tracer's pool (Take) and given back on every exit path.
struct EventPair {
  rt2_tracer* t;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  explicit EventPair(rt2_tracer* tracer) : t(tracer) {}
  EventPair(const EventPair&) = delete;
  EventPair& operator=(const EventPair&) = delete;
  ~EventPair() {
    if (e0) t->event_pool.push_back(e0);
    if (e1) t->event_pool.push_back(e1);
  }
  bool Take() {
    e0 = TakeEvent(t);
    e1 = TakeEvent(t);
    return e0 && e1;
  }
};

}  // namespace rt2::detail
