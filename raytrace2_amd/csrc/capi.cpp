// capi.cpp — implementation of include/rt2.h: scene handles, the device-side RayTracer's lifecycle, settings,
// render launches, readbacks and stats, and the host utilities. Device memory is owned by the tracer's buffers
// (tracer.h); the caller owns host buffers. The launch arithmetic is launch_plan.h; the noise estimate and
// adaptive sampling, the filters and the multi-GPU entry points are capi_estimate.cpp, capi_filter.cpp and
// capi_multi.cpp.
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "launch_plan.h"
#include "tracer.h"

namespace rt2 {
bool WriteImage(const float* pixels, int w, int h, const std::string& path, bool png, std::string& err);  // image.cpp
}  // namespace rt2

using namespace rt2;
using namespace rt2::detail;

namespace rt2::detail {

static thread_local std::string g_err;  // rt2_last_error's text

int Fail(int code, const std::string& m) {
  g_err = m;
  return code;
}
int HipFail(hipError_t e, const char* what) {
  return Fail(RT2_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

int LocalRows(int h, int band_h, int rank, int world) {
  int n = 0;
  for (int y = 0; y < h; y++)
    if (BandRank(y / band_h, world) == rank) n++;
  return n;
}

// The tracer's device buffers in three groups, each listed once, in the order it is freed: the free functions
// below and DeviceBytes both go through these lists, so a buffer added to one is freed and counted. f takes a
// DeviceBuffer or a Recon (Release, BytesOf); T: rt2_tracer or const rt2_tracer. First the scene program and tables and the small per-tracer buffers, in the order rt2_tracer_create uploads them.
template <typename T, typename Fn>
static void ForSceneBuffers(T* t, Fn&& f) {
  for (auto* d : {&t->d_nodes, &t->d_materials, &t->d_textures, &t->d_perlin_vec, &t->d_perlin_perm, &t->d_lin,
                  &t->d_lin_wide, &t->d_lind, &t->d_hit, &t->d_flat_wide, &t->d_flat_cert, &t->d_work, &t->d_stats,
                  &t->d_query_rays, &t->d_query_hits, &t->d_radiance_slots})
    f(*d);
}
// The frame buffers of the local rows, with their reconstruction.
template <typename T, typename Fn>
static void ForFrameBuffers(T* t, Fn&& f) {
  for (auto* d : {&t->d_accum, &t->d_pixels, &t->d_ray_counts, &t->d_moment2, &t->d_noise, &t->d_counts, &t->d_active,
                  &t->d_over, &t->d_list, &t->d_slot_of, &t->d_ad_scratch, &t->d_check_sum})
    f(*d);
  f(t->recon);
}
// A root's gathered image, its estimate (capi_multi.cpp) and its reconstruction: the history goes with the image.
template <typename T, typename Fn>
static void ForImageBuffers(T* t, Fn&& f) {
  for (auto* d : {&t->d_stacks, &t->d_image, &t->d_image_nc, &t->d_image_px, &t->d_stacks2, &t->d_image_var,
                  &t->d_stacks_n, &t->d_image_n})
    f(*d);
  f(t->image_recon);
}
static void Release(DeviceBuffer& d) { d.reset(); }
static void Release(Recon& r) { r.Free(); }
static size_t BytesOf(const DeviceBuffer& d) { return d.bytes(); }
static size_t BytesOf(const Recon& r) { return r.Bytes(); }

void FreeImage(rt2_tracer* t) {
  ForImageBuffers(t, [](auto& d) { Release(d); });
  t->image_frame = -1;
  t->estimate_frame = -1;
  t->image_counts = false;
}

static void FreeFrame(rt2_tracer* t) {
  for (auto& sl : t->slots) (void)sl.samples.reset();  // stream-ordered (LaunchFrames)
  ForFrameBuffers(t, [](auto& d) { Release(d); });
  FreeImage(t);
}

// Device bytes this tracer holds now: the scene program and small buffers with the clock ring, the frame
// buffers, both launch slots' sample buffers and chunk tables, and a root's gathered image.
static size_t DeviceBytes(const rt2_tracer* t) {
  size_t b = t->d_clock.bytes();
  const auto add = [&b](const auto& d) { b += BytesOf(d); };
  ForSceneBuffers(t, add);
  ForFrameBuffers(t, add);
  ForImageBuffers(t, add);
  for (const auto& sl : t->slots) b += sl.samples.bytes() + sl.chunks.bytes();
  return b;
}

void NoteDeviceBytes(rt2_tracer* t) { t->device_bytes_peak = std::max(t->device_bytes_peak, DeviceBytes(t)); }

int Realloc(rt2_tracer* t) {
  FreeFrame(t);
  t->local_rows = t->height > 0 ? LocalRows(t->height, BandH(t), t->rank, t->world) : 0;
  size_t n = (size_t)t->width * (size_t)AllocRows(t);
  if (n == 0) return RT2_OK;
  HIP_TRY(t->d_accum.Alloc(n * 3 * sizeof(float)));
  HIP_TRY(t->d_pixels.Alloc(n * 4));
  if (t->ray_counts_on) HIP_TRY(t->d_ray_counts.Alloc(n * sizeof(uint32_t)));
  if (t->moments_on) HIP_TRY(t->d_moment2.Alloc(n * 3 * sizeof(float)));
  if (t->adaptive_on) {
    const size_t tiles = AdaptiveTiles(t->width, std::max(t->local_rows, 1));
    const size_t blocks = AdaptiveBlocks((uint32_t)n);
    // the padded stack, like d_accum (n counts AllocRows): a gather with image_adaptive on sends BandRowsMax rows
    // of counts from every rank, and a rank with fewer rows must not be read past its end; ResetFrame zeroes the
    // padding and no kernel writes it
    HIP_TRY(t->d_counts.Alloc(n * sizeof(uint32_t)));
    HIP_TRY(t->d_active.Alloc(n));
    HIP_TRY(t->d_over.Alloc(n));
    HIP_TRY(t->d_list.Alloc((n + 64) * sizeof(uint32_t)));
    HIP_TRY(t->d_slot_of.Alloc(n * sizeof(uint32_t)));
    HIP_TRY(t->d_ad_scratch.Alloc(tiles * 12 + 4 + blocks * sizeof(AdaptivePartial) + sizeof(AdaptiveTotals) + 16));
  }
  NoteDeviceBytes(t);
  return RT2_OK;
}

int ResetFrame(rt2_tracer* t) {
  size_t n = (size_t)t->width * (size_t)AllocRows(t);
  t->frame_idx = 0;
  t->queued = 0;  // queued frames would only be accumulated and zeroed again
  t->image_frame = -1;
  t->estimate_frame = -1;
  t->n_active = (uint32_t)((size_t)t->width * (size_t)t->local_rows);  // adaptive: every pixel active again
  t->last_check = {};
  if (n == 0) return RT2_OK;
  HIP_TRY(hipSetDevice(t->device));
  HIP_TRY(hipMemsetAsync(t->d_accum.get<float>(), 0, n * 3 * sizeof(float), t->stream));
  HIP_TRY(hipMemsetAsync(t->d_pixels.get<uint8_t>(), 0, n * 4, t->stream));
  if (t->d_ray_counts) HIP_TRY(hipMemsetAsync(t->d_ray_counts.get<uint32_t>(), 0, n * sizeof(uint32_t), t->stream));
  if (t->d_moment2) HIP_TRY(hipMemsetAsync(t->d_moment2.get<float>(), 0, n * 3 * sizeof(float), t->stream));
  if (t->d_counts) {
    HIP_TRY(hipMemsetAsync(t->d_counts.get<uint32_t>(), 0, n * sizeof(uint32_t), t->stream));
    HIP_TRY(hipMemsetAsync(t->d_active.get<uint8_t>(), 1, n, t->stream));
  }
  return RT2_OK;
}

hipEvent_t TakeEvent(rt2_tracer* t) {
  if (!t->event_pool.empty()) {
    hipEvent_t e = t->event_pool.back();
    t->event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

static int DrainEvents(rt2_tracer* t) {
  if (!t->pending.empty() || !t->gpending.empty() || !t->rpending.empty()) t->host_waits++;
  if (!t->pending.empty()) {
    // every render launch is followed by its accumulate on the tracer stream, so a copy queued there
    // reads the clocks of all of them
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(hipMemcpyAsync(t->h_clock, t->d_clock.get<unsigned long long>(), 2 * sizeof(unsigned long long) * kClockRing,
                           hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    std::vector<std::pair<unsigned long long, unsigned long long>> iv;
    for (uint32_t k : t->pending) {
      const unsigned long long s = ~t->h_clock[2 * k], e = t->h_clock[2 * k + 1];
      if (t->h_clock[2 * k] != 0ull && e >= s) iv.emplace_back(s, e);
    }
    std::sort(iv.begin(), iv.end());
    const double ms_per_tick = 1.0 / t->clock_khz;
    for (const auto& x : iv) {
      t->launch_ms_sum += (double)(x.second - x.first) * ms_per_tick;
      const unsigned long long from = std::max(x.first, t->busy_end);
      if (x.second > from) t->kernel_ms += (double)(x.second - from) * ms_per_tick;
      t->busy_end = std::max(t->busy_end, x.second);
    }
  }
  t->pending.clear();
  for (auto& pr : t->gpending) {
    HIP_TRY(hipEventSynchronize(pr.second));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, pr.first, pr.second));
    t->gather_ms += ms;
    t->event_pool.push_back(pr.first);
    t->event_pool.push_back(pr.second);
  }
  t->gpending.clear();
  for (auto& pr : t->rpending) {
    HIP_TRY(hipEventSynchronize(pr.second));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, pr.first, pr.second));
    t->readback_ms += ms;
    t->event_pool.push_back(pr.first);
    t->event_pool.push_back(pr.second);
  }
  t->rpending.clear();
  return RT2_OK;
}

int Sync(rt2_tracer* t) {
  int rc = Flush(t);
  if (rc != RT2_OK) return rc;
  HIP_TRY(hipSetDevice(t->device));
  t->host_waits++;
  HIP_TRY(hipStreamSynchronize(t->stream));
  return DrainEvents(t);
}

}  // namespace rt2::detail

namespace {

// Flush before a setting that changes how the queued frames render.
template <typename T>
int FlushIfChanged(rt2_tracer* t, const T& cur, const T& next) {
  return cur == next ? RT2_OK : Flush(t);
}

void Put3(float* d, vec3 v) {
  d[0] = v.x;
  d[1] = v.y;
  d[2] = v.z;
}

}  // namespace

extern "C" {

const char* rt2_last_error(void) { return g_err.c_str(); }
#ifndef RT2_KERNEL_SHA
#define RT2_KERNEL_SHA "unknown"
#endif
// "rt2-mi355x 0.1 (gfx950) kernel <sha1 of the render kernel's sources (Makefile KERNEL_SHA), 12 hex digits>"
const char* rt2_version(void) { return "rt2-mi355x 0.1 (gfx950) kernel " RT2_KERNEL_SHA; }

int rt2_scene_load(const char* path, uint64_t seed, rt2_scene** out) {
  if (!path || !out) return Fail(RT2_ERR_INVALID, "rt2_scene_load: null argument");
  *out = nullptr;
  auto s = std::make_unique<rt2_scene>();
  std::string err;
  if (!LoadScene(path, seed, s->scene, err)) {
    bool io = err.rfind("Failed to open", 0) == 0;
    return Fail(io ? RT2_ERR_IO : RT2_ERR_SCENE, err);
  }
  const char* na = getenv("RT2_NO_LIST_ACCEL");
  const bool accel = !(na && na[0] == '1');
  if (!CompileScene(s->scene, s->compiled, err, accel)) return Fail(RT2_ERR_SCENE, err);
  *out = s.release();
  return RT2_OK;
}

void rt2_scene_free(rt2_scene* s) { delete s; }

int rt2_scene_get_info(const rt2_scene* s, rt2_scene_info* o) {
  if (!s || !o) return Fail(RT2_ERR_INVALID, "rt2_scene_get_info: null argument");
  const Scene& sc = s->scene;
  const CompiledScene& c = s->compiled;
  o->dims_x = sc.dims_x;
  o->dims_y = sc.dims_y;
  o->n_materials = (int)sc.materials.size();
  o->n_textures = (int)sc.textures.size();
  o->n_primitives = (int)sc.primitives.size();
  o->n_top_nodes = (int)sc.top.size();
  Put3(o->background, sc.background);
  o->legacy_schema = sc.legacy_schema ? 1 : 0;
  o->bvh_nodes = c.bvh_nodes;
  o->quads = c.quads;
  o->spheres = c.spheres;
  o->lists = c.lists;
  o->xforms = c.xforms;
  o->media = c.media;
  o->max_stack = c.max_stack;
  o->bvh_depth = c.bvh_depth;
  o->node_bytes = (uint64_t)c.nodes.size() * sizeof(float);
  o->acc_lists = c.acc_lists;
  o->acc_nodes = c.acc_nodes;
  o->linear_steps = (int)(c.lin.size() / 4);
  o->origins_bounded = c.origins_bounded ? 1 : 0;
  o->box_steps = c.box_steps;
  o->hit_table_bytes = (int)(c.hit.size() * sizeof(float));
  o->flat_steps = c.flat_steps;
  return RT2_OK;
}

int rt2_scene_materials(const rt2_scene* s, float* out, int cap) {
  if (!s) return Fail(RT2_ERR_INVALID, "null scene");
  int n = (int)s->scene.materials.size();
  for (int i = 0; i < n && i < cap && out; i++) {
    const MaterialDesc& m = s->scene.materials[(size_t)i];
    float* r = out + 8 * i;
    r[0] = (float)m.type;
    r[1] = m.albedo.x;
    r[2] = m.albedo.y;
    r[3] = m.albedo.z;
    r[4] = m.fuzz;
    r[5] = m.refraction_index;
    r[6] = (float)m.tex_idx;
    r[7] = 0;
  }
  return n;
}

int rt2_scene_textures(const rt2_scene* s, float* out, int cap) {
  if (!s) return Fail(RT2_ERR_INVALID, "null scene");
  int n = (int)s->scene.textures.size();
  for (int i = 0; i < n && i < cap && out; i++) {
    const TextureDesc& t = s->scene.textures[(size_t)i];
    float* r = out + 8 * i;
    r[0] = (float)t.type;
    r[1] = t.albedo.x;
    r[2] = t.albedo.y;
    r[3] = t.albedo.z;
    r[4] = t.type == kTexChecker ? t.inv_scale : t.scale;
    r[5] = (float)t.even;
    r[6] = (float)t.odd;
    r[7] = (float)t.noise_type;
  }
  return n;
}

int rt2_scene_perlin(const rt2_scene* s, int tex, float* vec, int* perm) {
  if (!s || tex < 0 || tex >= (int)s->scene.textures.size()) return Fail(RT2_ERR_INVALID, "bad texture index");
  const TextureDesc& t = s->scene.textures[(size_t)tex];
  if (t.type != kTexNoise) return Fail(RT2_ERR_INVALID, "not a noise texture");
  int pc = t.point_count;
  for (int i = 0; i < pc; i++) {
    if (vec) Put3(vec + 3 * i, t.perlin_vec[(size_t)i]);
    if (perm) {
      perm[i] = t.perm_x[(size_t)i];
      perm[pc + i] = t.perm_y[(size_t)i];
      perm[2 * pc + i] = t.perm_z[(size_t)i];
    }
  }
  return pc;
}

int rt2_scene_get_camera(const rt2_scene* s, rt2_camera_desc* o) {
  if (!s || !o) return Fail(RT2_ERR_INVALID, "null argument");
  const Camera& c = s->scene.cam;
  Put3(o->center, c.center_);
  Put3(o->look_at, c.lookat_);
  Put3(o->view_up, c.view_up_);
  o->vfov = c.vfov_;
  o->defocus_angle = c.defocus_angle_;
  o->focus_distance = c.focus_dist_;
  return RT2_OK;
}

int rt2_scene_set_camera(rt2_scene* s, const rt2_camera_desc* c) {
  if (!s || !c) return Fail(RT2_ERR_INVALID, "null argument");
  Camera& cam = s->scene.cam;
  cam.SetCenter(vec3{c->center[0], c->center[1], c->center[2]});
  cam.SetLookAt(vec3{c->look_at[0], c->look_at[1], c->look_at[2]});
  cam.SetViewUp(vec3{c->view_up[0], c->view_up[1], c->view_up[2]});
  cam.SetFOV(c->vfov);
  cam.SetDefocusAngle(c->defocus_angle);
  cam.SetFocusDistance(c->focus_distance);
  return RT2_OK;
}

int rt2_camera_params(const rt2_scene* s, int w, int h, int spp, float* out) {
  if (!s || !out || w <= 0 || h <= 0 || spp <= 0) return Fail(RT2_ERR_INVALID, "bad camera query");
  Camera c = s->scene.cam;
  c.SetDims(w, h);
  c.SetSamplesPerPixel(spp);
  CameraParams p = c.Params();
  memcpy(out, p.pixel00, 3 * sizeof(float));
  memcpy(out + 3, p.du, 3 * sizeof(float));
  memcpy(out + 6, p.dv, 3 * sizeof(float));
  memcpy(out + 9, p.center, 3 * sizeof(float));
  memcpy(out + 12, p.defocus_u, 3 * sizeof(float));
  memcpy(out + 15, p.defocus_v, 3 * sizeof(float));
  out[18] = p.defocus_angle;
  out[19] = p.recip_sqrt_spp;
  out[20] = (float)p.sqrt_spp;
  return RT2_OK;
}

int rt2_camera_load(const char* path, rt2_camera_desc* o) {
  if (!path || !o) return Fail(RT2_ERR_INVALID, "null argument");
  Camera c;
  std::string err;
  if (!LoadCameraFile(path, c, err)) return Fail(RT2_ERR_IO, err);
  Put3(o->center, c.center_);
  Put3(o->look_at, c.lookat_);
  Put3(o->view_up, c.view_up_);
  o->vfov = c.vfov_;
  o->defocus_angle = c.defocus_angle_;
  o->focus_distance = c.focus_dist_;
  return RT2_OK;
}

int rt2_camera_write(const rt2_camera_desc* d, const char* path) {
  if (!d || !path) return Fail(RT2_ERR_INVALID, "null argument");
  Camera c;
  c.SetCenter(vec3{d->center[0], d->center[1], d->center[2]});
  c.SetLookAt(vec3{d->look_at[0], d->look_at[1], d->look_at[2]});
  c.SetViewUp(vec3{d->view_up[0], d->view_up[1], d->view_up[2]});
  c.SetFOV(d->vfov);
  c.SetDefocusAngle(d->defocus_angle);
  c.SetFocusDistance(d->focus_distance);
  std::string err;
  if (!WriteCameraFile(c, path, err)) return Fail(RT2_ERR_IO, err);
  return RT2_OK;
}

int rt2_settings_load(const char* path, rt2_app_settings* o) {
  if (!path || !o) return Fail(RT2_ERR_INVALID, "null argument");
  AppSettings a;
  std::string err;
  if (!LoadAppSettingsFile(path, a, err)) return Fail(RT2_ERR_IO, err);
  o->render_once = a.render_once;
  o->save_after_render_once = a.save_after_render_once;
  o->num_samples = a.num_samples;
  o->max_depth = a.max_depth;
  o->render_window = a.render_window;
  return RT2_OK;
}

int rt2_tracer_create(const rt2_scene* s, int device, rt2_tracer** out) {
  if (!s || !out) return Fail(RT2_ERR_INVALID, "rt2_tracer_create: null argument");
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) return Fail(RT2_ERR_HIP, "no HIP device available");
  if (device < 0 || device >= ndev) return Fail(RT2_ERR_INVALID, "device index out of range");
  auto t = std::make_unique<rt2_tracer>();
  t->device = device;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreateWithFlags(&t->own_stream, hipStreamNonBlocking));
  t->stream = t->own_stream;
  for (auto& sl : t->slots) {
    HIP_TRY(hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&sl.rendered, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&sl.consumed, hipEventDisableTiming));
  }
  if (const char* e = getenv("RT2_PIPELINE")) t->pipeline = e[0] != '0';
  const CompiledScene& c = s->compiled;
  HIP_TRY(t->d_nodes.Upload(c.nodes.data(), c.nodes.size() * sizeof(float)));
  std::vector<float> mats = c.materials;
  if (mats.empty()) mats.assign(8, 0.0f);
  HIP_TRY(t->d_materials.Upload(mats.data(), mats.size() * sizeof(float)));
  HIP_TRY(t->d_textures.Upload(c.textures.data(), c.textures.size() * sizeof(float)));
  HIP_TRY(t->d_perlin_vec.Upload(c.perlin_vec.data(), c.perlin_vec.size() * sizeof(float)));
  HIP_TRY(t->d_perlin_perm.Upload(c.perlin_perm.data(), c.perlin_perm.size() * sizeof(int)));
  if (!c.lin.empty()) {
    HIP_TRY(t->d_lin.Upload(c.lin.data(), c.lin.size() * sizeof(uint32_t)));
    HIP_TRY(t->d_lin_wide.Upload(c.lin_wide.data(), c.lin_wide.size() * sizeof(uint32_t)));
    HIP_TRY(t->d_lind.Upload(c.lind.data(), c.lind.size() * sizeof(float)));
    t->lin_len = (uint32_t)(c.lin.size() / 4);
    if (!c.hit.empty()) HIP_TRY(t->d_hit.Upload(c.hit.data(), c.hit.size() * sizeof(float)));
    if (!c.flat_wide.empty() && c.flat_cert.size() == c.lind.size() && c.lin_xform_depth <= 1) {
      HIP_TRY(t->d_flat_wide.Upload(c.flat_wide.data(), c.flat_wide.size() * sizeof(uint32_t)));
      HIP_TRY(t->d_flat_cert.Upload(c.flat_cert.data(), c.flat_cert.size() * sizeof(float)));
      t->flat_mode = c.flat_mode;
    }
  }
  HIP_TRY(t->d_work.Alloc(128));
  HIP_TRY(t->d_clock.Alloc(2 * sizeof(unsigned long long) * kClockRing));
  HIP_TRY(hipMemset(t->d_clock.get<void>(), 0, t->d_clock.bytes()));
  HIP_TRY(hipHostMalloc((void**)&t->h_clock, t->d_clock.bytes(), hipHostMallocDefault));
  {
    int khz = 0;  // the constant clock s_memrealtime counts (100 MHz on MI355X)
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0)
      t->clock_khz = (double)khz;
  }
  HIP_TRY(t->d_stats.Alloc(kStatsSlots * sizeof(unsigned long long)));
  HIP_TRY(hipMemset(t->d_stats.get<void>(), 0, t->d_stats.bytes()));
  t->root = c.root;
  t->node_records = (uint32_t)(c.nodes.size() / 4);
  t->hot_records = c.hot_records;
  t->features = c.features;
  t->n_materials = (int)(c.materials.size() / 8);
  t->max_stack = c.max_stack;
  t->stack_ok = c.stack_ok;
  t->flat_xforms = c.lin_xform_depth <= 1;
  t->origins_bounded = c.origins_bounded;
  Put3(t->background, s->scene.background);
  t->camera = s->scene.cam;
  HIP_TRY(hipDeviceGetAttribute(&t->cus, hipDeviceAttributeMultiprocessorCount, device));
  HIP_TRY(hipDeviceGetAttribute(&t->lds_per_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, device));
  if (const char* e = getenv("RT2_NO_LDS")) t->use_lds = e[0] == '0';
  if (const char* e = getenv("RT2_NO_LINEAR")) t->use_linear = e[0] == '0';
  if (const char* e = getenv("RT2_NO_HYBRID")) t->use_hybrid = e[0] == '0';
  if (const char* e = getenv("RT2_FORCE_HYBRID")) t->force_hybrid = e[0] == '1';
  if (const char* e = getenv("RT2_HYBRID_RECORDS")) t->hybrid_cap = atoi(e);
  if (const char* e = getenv("RT2_CHUNK_MAX")) t->chunk_max = std::max(1, atoi(e));
  if (const char* e = getenv("RT2_CHUNK_ALIGN")) t->chunk_align = e[0] != '0';
  if (const char* e = getenv("RT2_FRAME_TILES")) t->frame_tiles_env = e[0] == '1' ? 1 : 0;
  if (const char* e = getenv("RT2_FRAME_TILE_LEN")) t->frame_tile_len = std::max(1, std::min(atoi(e), 64));
  // App.cpp:122-125,157: scene dims when present, else the window default 1600x900
  int w = s->scene.dims_x > 0 && s->scene.dims_y > 0 ? s->scene.dims_x : 1600;
  int h = s->scene.dims_x > 0 && s->scene.dims_y > 0 ? s->scene.dims_y : 900;
  const int rc = rt2_tracer_on_resize(t.get(), w, h);
  if (rc != RT2_OK) return rc;
  *out = t.release();
  return RT2_OK;
}

void rt2_tracer_destroy(rt2_tracer* t) {
  if (!t) return;
  for (rt2_tracer* p : t->parts) rt2_tracer_destroy(p);
  delete t;
}

}  // extern "C"

// Everything the tracer holds on its GPU, in this order (not the members'): the stream is idle before the
// communicator, the events and the buffers go; the streams go last. Also the way out of every early return
// of rt2_tracer_create. A multi tracer's facade holds nothing here (its parts do).
rt2_tracer::~rt2_tracer() {
  if (!own_stream) return;  // the facade, or a tracer whose creation failed before its first stream
  (void)hipSetDevice(device);
  if (stream) (void)hipStreamSynchronize(stream);
  if (comm) (void)ncclCommDestroy(comm);
  for (auto& pr : gpending) {
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  for (auto& pr : rpending) {
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  if (stream) (void)hipStreamSynchronize(stream);
  for (hipEvent_t e : event_pool) (void)hipEventDestroy(e);
  for (KernelTimer* k : {&recon.present_timer, &image_recon.present_timer, &query_timer, &ambient_timer, &radiance_timer})
    k->Release();
  d_clock.reset();
  if (h_clock) (void)hipHostFree(h_clock);
  if (h_check) (void)hipHostFree(h_check);
  FreeFrame(this);
  ForSceneBuffers(this, [](auto& d) { Release(d); });
  for (auto& sl : slots) {
    (void)sl.chunks.reset();
    if (sl.stream) (void)hipStreamSynchronize(sl.stream);
  }
  if (stream) (void)hipStreamSynchronize(stream);
  for (auto& st : staging) {
    (void)hipEventDestroy(st.done);
    (void)hipHostFree(st.p);
  }
  if (own_stream) (void)hipStreamDestroy(own_stream);
  for (auto& sl : slots) {
    if (sl.rendered) (void)hipEventDestroy(sl.rendered);
    if (sl.consumed) (void)hipEventDestroy(sl.consumed);
    if (sl.stream) (void)hipStreamDestroy(sl.stream);
  }
}

extern "C" {

int rt2_tracer_set_stream(rt2_tracer* t, void* s) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  if (IsMulti(t)) {
    if (t->parts.size() != 1) return Fail(RT2_ERR_INVALID, "set_stream: a multi-GPU tracer owns one stream per GPU");
    return rt2_tracer_set_stream(t->parts[0], s);
  }
  int rc = Sync(t);
  if (rc != RT2_OK) return rc;
  t->stream = s ? (hipStream_t)s : t->own_stream;
  return RT2_OK;
}

int rt2_tracer_set_max_depth(rt2_tracer* t, int d) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  RT2_FORWARD(t, rt2_tracer_set_max_depth(p, d));
  // RayTracer::max_depth is a size_t (RayTracer.hpp:32); the kernel keeps it in 16 bits
  if (d > 0xFFFF) return Fail(RT2_ERR_INVALID, "max_depth must be at most 65535");
  int rc = FlushIfChanged(t, t->max_depth, d < 0 ? 0 : d);
  if (rc != RT2_OK) return rc;
  t->max_depth = d < 0 ? 0 : d;
  return RT2_OK;
}

int rt2_tracer_set_samples_per_pixel(rt2_tracer* t, int spp) {
  if (!t || spp <= 0) return Fail(RT2_ERR_INVALID, "samples_per_pixel must be positive");
  RT2_FORWARD(t, rt2_tracer_set_samples_per_pixel(p, spp));
  int rc = FlushIfChanged(t, t->camera.SamplesPerPixel(), spp);
  if (rc != RT2_OK) return rc;
  t->camera.SetSamplesPerPixel(spp);
  return RT2_OK;
}

int rt2_tracer_set_seed(rt2_tracer* t, uint64_t seed) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  RT2_FORWARD(t, rt2_tracer_set_seed(p, seed));
  int rc = FlushIfChanged(t, t->seed, seed);
  if (rc != RT2_OK) return rc;
  t->seed = seed;
  return RT2_OK;
}

int rt2_tracer_set_partition(rt2_tracer* t, int band_h, int rank, int world) {
  if (!t || band_h < 0 || world < 1 || rank < 0 || rank >= world)
    return Fail(RT2_ERR_INVALID, "bad partition (need band_h >= 0, 0 <= rank < world)");
  if (IsMulti(t)) return Fail(RT2_ERR_INVALID, "set_partition: a multi-GPU tracer partitions itself");
  if (t->comm && (rank != t->rank || world != t->world || band_h != t->band_h))
    return Fail(RT2_ERR_INVALID, "set_partition: the tracer is joined to a communicator with another partition");
  t->queued = 0;  // the partition change resets the frame
  int rc = Sync(t);
  if (rc != RT2_OK) return rc;
  t->band_h = band_h;
  t->rank = rank;
  t->world = world;
  if ((rc = Realloc(t)) != RT2_OK) return rc;
  return ResetFrame(t);
}

int rt2_tracer_set_launch_frames(rt2_tracer* t, int n) {
  if (!t || n < 0) return Fail(RT2_ERR_INVALID, "frames_per_launch must be >= 0");
  RT2_FORWARD(t, rt2_tracer_set_launch_frames(p, n));
  t->launch_frames = n;
  return RT2_OK;
}

int rt2_tracer_set_work_split(rt2_tracer* t, int items_per_lane) {
  if (!t || items_per_lane < 0) return Fail(RT2_ERR_INVALID, "items_per_lane must be >= 0");
  RT2_FORWARD(t, rt2_tracer_set_work_split(p, items_per_lane));
  t->work_split = items_per_lane;
  return RT2_OK;
}

int rt2_tracer_set_batch_max(rt2_tracer* t, int items) {
  if (!t || items < 1) return Fail(RT2_ERR_INVALID, "batch must be >= 1");
  RT2_FORWARD(t, rt2_tracer_set_batch_max(p, items));
  t->batch_max = items;
  return RT2_OK;
}

int rt2_tracer_set_sample_budget(rt2_tracer* t, uint64_t bytes) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  RT2_FORWARD(t, rt2_tracer_set_sample_budget(p, bytes));
  t->sample_budget = (size_t)bytes;
  return RT2_OK;
}

int rt2_tracer_last_launch(const rt2_tracer* t, int* grid, int* chunk_frames, int* variant) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  if (IsMulti(t)) return rt2_tracer_last_launch(t->parts[0], grid, chunk_frames, variant);
  if (grid) *grid = t->last_grid;
  if (chunk_frames) *chunk_frames = t->last_chunk_frames;
  if (variant) *variant = t->last_variant;
  return RT2_OK;
}

int rt2_tracer_on_resize(rt2_tracer* t, int w, int h) {
  if (!t || w <= 0 || h <= 0) return Fail(RT2_ERR_INVALID, "dims must be positive");
  if (w > 65535 || h > 65535) return Fail(RT2_ERR_INVALID, "dims must be at most 65535");
  // the kernel's pixel index (Philox pixel word, magic division by the width) stays below 2^31
  if ((int64_t)w * h >= (int64_t)1 << 31) return Fail(RT2_ERR_INVALID, "width * height must be below 2^31");
  if (IsMulti(t)) {
    t->width = w;
    t->height = h;
    return ForParts(t, [&](rt2_tracer* p) { return rt2_tracer_on_resize(p, w, h); });
  }
  t->queued = 0;  // OnResize resets the frame
  int rc = Sync(t);
  if (rc != RT2_OK) return rc;
  t->width = w;
  t->height = h;
  t->camera.SetDims(w, h);
  if ((rc = Realloc(t)) != RT2_OK) return rc;
  return ResetFrame(t);
}

int rt2_tracer_reset(rt2_tracer* t) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  RT2_FORWARD(t, rt2_tracer_reset(p));
  return ResetFrame(t);
}

int rt2_tracer_set_camera(rt2_tracer* t, const rt2_camera_desc* c) {
  if (!t || !c) return Fail(RT2_ERR_INVALID, "null argument");
  RT2_FORWARD(t, rt2_tracer_set_camera(p, c));
  const Camera& cur = t->camera;
  const vec3 center{c->center[0], c->center[1], c->center[2]};
  const vec3 look{c->look_at[0], c->look_at[1], c->look_at[2]};
  const vec3 up{c->view_up[0], c->view_up[1], c->view_up[2]};
  auto same3 = [](vec3 a, vec3 b) { return memcmp(&a, &b, sizeof(vec3)) == 0; };
  const bool same = same3(cur.center_, center) && same3(cur.lookat_, look) && same3(cur.view_up_, up) &&
                    memcmp(&cur.vfov_, &c->vfov, 4) == 0 && memcmp(&cur.defocus_angle_, &c->defocus_angle, 4) == 0 &&
                    memcmp(&cur.focus_dist_, &c->focus_distance, 4) == 0;
  if (same) return RT2_OK;  // the reference's lazy camera: nothing dirty, nothing to recompute
  int rc = Flush(t);        // queued frames render with the camera they were queued under
  if (rc != RT2_OK) return rc;
  t->camera.SetCenter(center);
  t->camera.SetLookAt(look);
  t->camera.SetViewUp(up);
  t->camera.SetFOV(c->vfov);
  t->camera.SetDefocusAngle(c->defocus_angle);
  t->camera.SetFocusDistance(c->focus_distance);
  return RT2_OK;
}

int rt2_tracer_get_camera(const rt2_tracer* t, rt2_camera_desc* o) {
  if (!t || !o) return Fail(RT2_ERR_INVALID, "null argument");
  if (IsMulti(t)) return rt2_tracer_get_camera(t->parts[0], o);
  const Camera& c = t->camera;
  Put3(o->center, c.center_);
  Put3(o->look_at, c.lookat_);
  Put3(o->view_up, c.view_up_);
  o->vfov = c.vfov_;
  o->defocus_angle = c.defocus_angle_;
  o->focus_distance = c.focus_dist_;
  return RT2_OK;
}

}  // extern "C"

namespace {
constexpr uint32_t kFrameTileMinSteps = 256;  // threaded programs longer than this use frame tiles

// Camera rays start within +-2^64 on every axis (center + the defocus disk's two half-axes): the
// kernel's rectangle test (compile.cpp RectAAWords) is exact for ray origins within +-2^100, and a
// scene the compiler gives that test lies within +-2^64 (Flattener::QuadAASpace). Checked only for
// scenes whose threaded program holds such a test (CompiledScene::origins_bounded).
bool CameraOriginsBounded(const CameraParams& c) {
  for (int k = 0; k < 3; k++)
    if (!(std::fabs((double)c.center[k]) + std::fabs((double)c.defocus_u[k]) + std::fabs((double)c.defocus_v[k]) <=
          0x1p64))
      return false;
  return true;
}
constexpr const char* kCameraRangeMsg = "camera origin or defocus disk outside +-2^64";

// Puts a launch's chunk table in its slot's table, ordered on the slot's render stream: the copy runs
// after the launches already queued there (which may still read the old table), from pinned staging
// memory, so the host never waits for the GPU (a multi-GPU tracer enqueues every GPU's launches at
// once). A launch repeating the slot's last schedule (the bench, a progressive loop's steady state)
// uploads nothing.
int UploadChunks(rt2_tracer* t, rt2_tracer::Slot& sl, const std::vector<uint32_t>& tab) {
  if (sl.chunks && tab == sl.chunks_host) return RT2_OK;
  const size_t bytes = tab.size() * sizeof(uint32_t);
  if (bytes > sl.chunks.bytes()) {
    // grow geometrically; stream-ordered free and allocation: the queued launches that read the old
    // table run first, and the host does not wait (hipFree would synchronize the device)
    const size_t cap = std::max(bytes, 2 * sl.chunks.bytes());
    sl.chunks_host.clear();
    HIP_TRY(sl.chunks.Alloc(cap, sl.stream));
  }
  // a staging buffer whose previous copy has run, else a new one
  rt2_tracer::Staging* st = nullptr;
  for (auto& c : t->staging) {
    if (c.bytes < bytes) continue;
    const hipError_t q = hipEventQuery(c.done);
    if (q == hipSuccess) {
      st = &c;
      break;
    }
    if (q != hipErrorNotReady) return HipFail(q, "hipEventQuery");
  }
  if (!st) {
    rt2_tracer::Staging c{nullptr, std::max<size_t>(bytes, 4096), nullptr};
    HIP_TRY(hipHostMalloc((void**)&c.p, c.bytes, hipHostMallocDefault));
    HIP_TRY(hipEventCreateWithFlags(&c.done, hipEventDisableTiming));
    t->staging.push_back(c);
    st = &t->staging.back();
  }
  memcpy(st->p, tab.data(), bytes);
  HIP_TRY(hipMemcpyAsync(sl.chunks.get<uint32_t>(), st->p, bytes, hipMemcpyHostToDevice, sl.stream));
  HIP_TRY(hipEventRecord(st->done, sl.stream));
  sl.chunks_host = tab;
  return RT2_OK;
}

}  // namespace

void rt2::detail::BaseParams(const rt2_tracer* t, const CameraParams& cam, RenderParams* out) {
  RenderParams& p = *out;
  memset(&p, 0, sizeof(p));
  p.nodes = t->d_nodes.get<void>();
  p.materials = t->d_materials.get<void>();
  p.textures = t->d_textures.get<void>();
  p.perlin_vec = t->d_perlin_vec.get<void>();
  p.perlin_perm = t->d_perlin_perm.get<int>();
  p.root = t->root;
  memcpy(p.background, t->background, sizeof(p.background));
  p.cam = cam;
  p.width = t->width;
  p.height = t->height;
  p.local_rows = t->local_rows;
  p.band_h = t->band_h > 0 ? t->band_h : t->height;
  p.rank = t->rank;
  p.world = t->world;
  p.seed_lo = (uint32_t)t->seed;
  p.seed_hi = (uint32_t)(t->seed >> 32);
  for (uint32_t r = 0; r < 10; r++) {
    p.philox_keys[2 * r] = p.seed_lo + r * 0x9E3779B9u;
    p.philox_keys[2 * r + 1] = p.seed_hi + r * 0xBB67AE85u;
  }
  p.stack_depth = t->max_stack;
}

namespace {

// What a launch stages in LDS and which tables it takes (the RenderParams fields of those names). The
// decisions ask the runtime for the kernels' occupancy (cached in the tracer: a query costs far more than a
// one-frame launch).
struct LdsPlan {
  uint32_t lds_nodes = 0, lds_partial = 0;
  const void* hit_table = nullptr;
  uint32_t hit_bytes = 0;
  const void *flat_wide = nullptr, *flat_cert = nullptr;
  uint32_t flat_mode = 0;
};
LdsPlan PlanLds(rt2_tracer* t, uint32_t lin_len, int stack_depth, int variant, bool counting, bool listed) {
  LdsPlan o;
  // Scene records in LDS: the whole scene when it fits; otherwise (stack traversal) the top levels
  // of the BVH — its node records are a breadth-first prefix of the record array — as many as fit
  // beside the traversal stack without lowering the occupancy the registers allow.
  // LDS room per workgroup that keeps the occupancy the registers allow (beside the stack)
  uint32_t room = 0;  // float4 records
  if (t->use_lds && !lin_len) {
    const int hkey = variant * 2 + (counting ? 1 : 0);
    if (t->hyb_key != hkey) {
      const size_t stack_bytes = (size_t)stack_depth * (size_t)RenderBlockSize() * 4;
      const int blocks = RenderBlocksPerCU(variant, kModeStackHybrid, counting, stack_bytes);
      const size_t per_block = (size_t)t->lds_per_cu / (size_t)std::max(1, blocks);
      t->hyb_records = (uint32_t)(per_block > stack_bytes ? (per_block - stack_bytes) / 16 : 0);
      t->hyb_key = hkey;
    }
    room = t->hyb_records;
  }
  // whole scene in LDS only when that costs no occupancy (measured on book 1 in stack mode: the
  // 32 KB scene in LDS limited it to 3 workgroups per CU, 3.9 Grays/s; the hybrid prefix 5.0)
  const bool lds = t->use_lds && !t->force_hybrid && !lin_len && t->node_records <= room &&
                   (size_t)t->node_records * 16 <= (size_t)kLdsSceneBytesMax;
  // Hybrid prefix: measured +20% on a 10^5-sphere field, but -15% on book 2, whose all-features
  // kernel already spills at its occupancy target; used for variants without media and transforms
  // unless forced (RT2_FORCE_HYBRID).
  const bool hybrid_variant = t->force_hybrid || !(RenderVariantFeatures(variant) & (kFeatMedium | kFeatXform));
  uint32_t hot = 0;
  if (!lds && hybrid_variant && t->use_lds && t->use_hybrid && t->hot_records > 0 && !lin_len) {
    hot = std::min<uint32_t>(std::min<uint32_t>(room, (uint32_t)(kLdsHotBytesMax / 16)), t->hot_records) & ~1u;
    if (t->hybrid_cap >= 0) hot = std::min(hot, (uint32_t)t->hybrid_cap & ~1u);
    if (hot < 2) hot = 0;
  }
  o.lds_nodes = lds ? t->node_records : hot;
  o.lds_partial = (!lds && hot) ? 1u : 0u;
  // The hit table in LDS, for the kernels that take it (render.hip HitTable()), when the kernel keeps
  // the occupancy it has without the table: the runtime is asked with and without it.
  // The flat program, for the launches whose kernel walks it (render.hip kFeatFlat: the Cornell kernel with
  // its hit table staged): decided per launch, so a counting launch, a launch over an active list or one
  // whose table is not staged walks the BVH program of the same scene.
  if (lin_len && t->d_hit && t->flat_xforms && RenderTakesHitTable(variant, kModeLinear, counting)) {
    const uint32_t hit_bytes = (uint32_t)t->d_hit.bytes();
    const auto fits = [&](bool flat_kernel) {  // (the list / flat kernel is asked about itself)
      const int hkey = variant * 4 + (listed ? 1 : 0) + (flat_kernel ? 2 : 0);
      if (t->hit_key != hkey) {
        t->hit_fits = RenderBlocksPerCU(variant, kModeLinear, counting, hit_bytes, listed, flat_kernel) >=
                      RenderBlocksPerCU(variant, kModeLinear, counting, 0, listed, flat_kernel);
        t->hit_key = hkey;
      }
      return t->hit_fits;
    };
    const bool flat_want = t->d_flat_wide && t->flat_mode != 0u && RenderTakesFlat(variant, kModeLinear, counting, listed);
    if (flat_want && fits(true)) {
      o.flat_wide = t->d_flat_wide.get<void>();
      o.flat_cert = t->d_flat_cert.get<void>();
      o.flat_mode = t->flat_mode;
    }
    if (o.flat_wide != nullptr || fits(false)) {
      o.hit_table = t->d_hit.get<void>();
      o.hit_bytes = hit_bytes;
    }
  }
  return o;
}

// Resident lanes of the launch's kernel instantiation (occupancy query cached: it costs far more than
// a one-frame launch).
int64_t ResidentLanes(rt2_tracer* t, const RenderParams& p, int variant, bool counting, bool listed) {
  const bool flat = p.flat_wide != nullptr;
  const size_t lds_bytes = RenderLdsBytes(p);
  const int okey = variant * 32 + RenderMode(p) * 2 + (counting ? 1 : 0) + (listed ? 8 : 0) + (flat ? 16 : 0);
  if (t->occ_key != okey || t->occ_lds != lds_bytes) {
    t->occ_blocks = RenderBlocksPerCU(variant, RenderMode(p), counting, lds_bytes, listed, flat);
    t->occ_key = okey;
    t->occ_lds = lds_bytes;
  }
  return (int64_t)t->cus * t->occ_blocks * RenderBlockSize();
}

// What LaunchFrames decides once for all the launches of a call.
struct LaunchSetup {
  bool listed;       // over the active list's n_slots slots (adaptive sampling), else over all the local pixels
  uint32_t n_slots;
  int variant;       // the kernel instantiation: feature set, with or without the counters
  bool counting;
  int64_t resident;  // its resident lanes
  size_t frame_bytes;  // one frame of samples
  int per_launch;    // most frames per launch
};
// One launch of the call: its frames and its chunk table's place in the call's tables.
struct Launch {
  int frame_begin, n_frames, first_len;
  uint32_t n_chunks;
  size_t table;  // offset in `tabs` (words)
};

// Step 1, the parameters every launch of the call shares: the base, the work tiles (or the active list's slots),
// the traversal, the kernel instantiation and what it stages in LDS.
int FillLaunchParams(rt2_tracer* t, LaunchSetup* s, RenderParams* out) {
  RenderParams& p = *out;
  BaseParams(t, t->camera.Params(), &p);  // RayTracer::Update → camera->Update() (RayTracer.cpp:56)
  if (p.cam.sqrt_spp <= 0) return Fail(RT2_ERR_INVALID, "samples_per_pixel gives sqrt_spp = 0");
  if (t->origins_bounded && !CameraOriginsBounded(p.cam)) return Fail(RT2_ERR_INVALID, kCameraRangeMsg);
  const TileGeometry g = PlanTiles(t->width, t->local_rows, p.band_h, t->world);
  p.tile_shift = g.tile_shift;
  p.tiles_x = g.tiles_x;
  p.tile_items = g.tile_items;
  p.div_tile_items = MakeMagic(p.tile_items);
  p.div_tiles_x = MakeMagic((uint32_t)p.tiles_x);
  p.div_band_h = MakeMagic((uint32_t)p.band_h);
  p.div_band_w = MakeMagic((uint32_t)p.band_h * (uint32_t)p.world);
  p.div_world = MakeMagic((uint32_t)p.world);
  p.div_width = MakeMagic((uint32_t)t->width);  // pixel index -> (x, y)
  p.local_pixels = s->n_slots;  // the sample buffer's pixels: all of them, or the list's slots
  if (s->listed) {  // items run over the slots padded to whole waves (RenderParams::active_list)
    p.tile_items = (s->n_slots + 63u) & ~63u;
    p.div_tile_items = MakeMagic(p.tile_items);
    p.active_list = t->d_list.get<uint32_t>();
    p.slot_of = t->d_slot_of.get<uint32_t>();
  }
  if (p.tile_items > 0x7FFFFFFFu)  // work items (and pixel indices) must stay below 2^31
    return Fail(RT2_ERR_INVALID, "image too large for one GPU (more than 2^31 pixels in a partition)");
  p.max_depth = t->max_depth;
  p.batch_max = (uint32_t)t->batch_max;
  p.ray_counts = t->d_ray_counts.get<uint32_t>();
  p.stats = t->d_stats.get<unsigned long long>();
  p.lin = t->d_lin.get<void>();
  p.lin_wide = t->d_lin_wide.get<void>();
  p.lind = t->d_lind.get<void>();
  p.lin_len = t->use_linear ? t->lin_len : 0u;
  p.flat_xforms = t->flat_xforms ? 1u : 0u;
  if (!p.lin_len && !t->stack_ok)
    return Fail(RT2_ERR_INVALID, "scene needs a traversal stack of " + std::to_string(t->max_stack) +
                                     " entries (kernel has " + std::to_string(kTraversalStack) +
                                     "): only the threaded traversal can render it");
  // Frame tiles (a wave's lanes trace one pixel's consecutive frames: paths from one pixel share
  // their first hit and start their secondary rays from nearly one point, so the lockstep walk of
  // a deep program serves more lanes per step) for deep threaded programs: measured with chunks of
  // up to 8 frames, book 2 (4,922 steps) +4 %, book 1 (995 steps) +4.5 %; Cornell (29 steps) -2 %,
  // where 8x8 pixel tiles are as coherent and the shorter chunks cost more item fetches.
  t->frame_tiles = t->frame_tiles_env >= 0 ? t->frame_tiles_env == 1 : (p.lin_len > kFrameTileMinSteps);
  // frame-tile items are g * 64 * local_pixels + ...: at least one 64-chunk group must stay below 2^31
  if ((uint64_t)p.local_pixels * 64u > 0x7FFFFFFFull) t->frame_tiles = false;
  uint32_t feats = t->features | (p.cam.defocus_angle > 0.0f ? (uint32_t)kFeatDefocus : 0u);
  s->variant = RenderVariant(feats);
  if (s->listed && !p.lin_len)  // the list kernels exist for the threaded traversal, the default mode
    return Fail(RT2_ERR_INVALID, "adaptive sampling needs the threaded traversal (the scene has none, or RT2_NO_LINEAR)");
  // per-record counters and per-pixel ray counts come from the counting kernel instantiation (same
  // arithmetic, extra counters); the product kernel keeps only the wave ray totals
  s->counting = t->stats_on || t->ray_counts_on;
  const LdsPlan l = PlanLds(t, p.lin_len, p.stack_depth, s->variant, s->counting, s->listed);
  p.lds_nodes = l.lds_nodes;
  p.lds_partial = l.lds_partial;
  p.hit_table = l.hit_table;
  p.hit_bytes = l.hit_bytes;
  p.flat_wide = l.flat_wide;
  p.flat_cert = l.flat_cert;
  p.flat_mode = l.flat_mode;
  t->last_hit_bytes = p.hit_bytes;
  t->last_variant = s->variant;
  return RT2_OK;
}

// Step 3, one launch on the next slot: waits, the slot's sample buffer and chunk table, the render kernel on
// the slot's stream and its accumulate on the tracer's.
int EnqueueLaunch(rt2_tracer* t, const LaunchSetup& s, const Launch& L, const std::vector<uint32_t>& tab, RenderParams& p) {
  rt2_tracer::Slot& sl = t->slots[t->next_slot];
  t->next_slot ^= 1;
  // The counting kernels add per-pixel ray counts that Reset() zeroes on the tracer stream: those
  // launches wait for it, as every launch does with RT2_PIPELINE=0.
  const bool serial = !t->pipeline || s.counting;
  // the slot's render stream waits for the accumulate that last read its sample buffer (or, serial,
  // for everything queued on the tracer stream so far); never for the other slot's render
  if (serial) {
    hipEvent_t e = TakeEvent(t);
    if (!e) return Fail(RT2_ERR_HIP, "event create failed");
    HIP_TRY(hipEventRecord(e, t->stream));
    HIP_TRY(hipStreamWaitEvent(sl.stream, e, 0));
    t->event_pool.push_back(e);
  } else if (sl.consumed_set) {
    HIP_TRY(hipStreamWaitEvent(sl.stream, sl.consumed, 0));
  }
  size_t need = SampleOctets((size_t)L.n_frames) * s.frame_bytes;
  if (need > sl.samples.bytes()) {
    // grow geometrically (progressive loops raise their frames per call a little at a time)
    need = std::max(need, std::min(2 * sl.samples.bytes(), SampleOctets((size_t)s.per_launch) * s.frame_bytes));
    // stream-ordered: the queued work still using the old buffer runs first; the host does not
    // wait (a multi-GPU tracer enqueues every GPU's render before any of them finishes)
    HIP_TRY(sl.samples.Alloc(need, sl.stream));
    NoteDeviceBytes(t);
  }
  p.samples = sl.samples.get<float>();
  int rc = UploadChunks(t, sl, tab);
  if (rc != RT2_OK) return rc;
  p.frame_begin = L.frame_begin;
  p.n_frames = L.n_frames;
  p.chunks = sl.chunks.get<uint32_t>();
  p.n_chunks = L.n_chunks;
  const LaunchItems it = PlanItems(L.n_chunks, p.tile_items, t->frame_tiles, p.local_pixels, s.resident, RenderBlockSize());
  if (t->frame_tiles) {
    p.frame_tiles = 1u;
    p.frame_tile = it.frame_tile;
    p.div_frame_tile = MakeMagic(p.frame_tile);
  }
  p.n_items = it.n_items;
  p.batch_div = it.batch_div;
  t->last_grid = it.grid;
  t->last_chunk_frames = L.first_len;
  p.work_counter = t->d_work.get<uint32_t>() + 16 * (&sl - t->slots);
  HIP_TRY(hipMemsetAsync(p.work_counter, 0, sizeof(uint32_t), sl.stream));
  // the launch's clock pair (RenderParams::launch_clock; read back by DrainEvents)
  const uint32_t ck = t->clock_next;
  t->clock_next = (t->clock_next + 1u) % (uint32_t)kClockRing;
  p.launch_clock = t->d_clock.get<unsigned long long>() + 2u * ck;
  HIP_TRY(hipMemsetAsync(p.launch_clock, 0, 2 * sizeof(unsigned long long), sl.stream));
  HIP_TRY(LaunchRender(p, s.variant, s.counting, it.grid, sl.stream));
  t->pending.push_back(ck);
  // accumulate in frame order on the tracer stream, after this launch (RayTracer.cpp:64)
  HIP_TRY(hipEventRecord(sl.rendered, sl.stream));
  HIP_TRY(hipStreamWaitEvent(t->stream, sl.rendered, 0));
  if (t->adaptive_on) {
    HIP_TRY(LaunchAccumulateList(sl.samples.get<float>(), s.listed ? t->d_list.get<uint32_t>() : nullptr,
                                 t->d_accum.get<float>(), t->d_moment2.get<float>(), t->d_counts.get<uint32_t>(),
                                 t->d_pixels.get<uint8_t>(), s.n_slots, p.n_frames, t->stream));
  } else {
    HIP_TRY(LaunchAccumulate(sl.samples.get<float>(), t->d_accum.get<float>(), t->d_moment2.get<float>(),
                             t->d_pixels.get<uint8_t>(), p.local_pixels, p.n_frames, p.frame_begin + p.n_frames, t->stream));
  }
  HIP_TRY(hipEventRecord(sl.consumed, t->stream));
  sl.consumed_set = true;
  t->launches++;
  t->paths += (uint64_t)p.n_frames * p.local_pixels;
  t->frame_idx += p.n_frames;
  // the ring's entries of unread launches must not be reused: read them back at half the ring
  if (t->pending.size() >= (size_t)kClockRing / 2) return DrainEvents(t);
  return RT2_OK;
}

// Launches frames [frame_idx, frame_idx + n_frames) now.
int LaunchFrames(rt2_tracer* t, int n_frames) {
  if (n_frames == 0 || t->local_rows == 0) {
    t->frame_idx += n_frames;
    return RT2_OK;
  }
  // Adaptive sampling: once a pixel has retired the launch runs over the list of the active pixels
  // (n_slots of them); with none left there is nothing to trace and only the frame index advances.
  const uint32_t all_pixels = (uint32_t)t->width * (uint32_t)t->local_rows;
  LaunchSetup s{};
  s.listed = t->adaptive_on && t->n_active < all_pixels;
  if (s.listed && t->n_active == 0) {
    t->frame_idx += n_frames;
    return RT2_OK;
  }
  s.n_slots = s.listed ? t->n_active : all_pixels;
  HIP_TRY(hipSetDevice(t->device));
  RenderParams p;
  int rc = FillLaunchParams(t, &s, &p);
  if (rc != RT2_OK) return rc;
  // Step 2, the plan: frames per launch (the caller's launch_frames, bounded by the sample-buffer budget) and
  // every launch's chunk schedule
  s.resident = ResidentLanes(t, p, s.variant, s.counting, s.listed);
  s.frame_bytes = (size_t)p.local_pixels * 3 * sizeof(float);
  s.per_launch = FramesPerLaunch(t->launch_frames, n_frames, t->sample_budget, s.frame_bytes, t->frame_tiles, p.local_pixels);
  const ChunkSettings cs{t->frame_tiles, t->frame_tile_len, t->work_split, t->chunk_max, t->chunk_align};
  std::vector<Launch> launches;
  std::vector<uint32_t> tabs;
  for (int done = 0, fb = (int)t->frame_idx; done < n_frames;) {
    Launch L{fb, std::min(s.per_launch, n_frames - done), 0, 0, tabs.size()};
    // Split each pixel's frames into chunks so that the launch has about work_split items per
    // resident lane: a persistent lane's last item is then short, and a small partition (a row
    // band of an 8-GPU split) still fills every CU. Samples land in the per-frame buffer, so the
    // accumulation order does not depend on the split.
    ChunkSchedule(cs, L.frame_begin, L.n_frames, p.tile_items, s.resident, p.cam.sqrt_spp, tabs, &L.n_chunks, &L.first_len);
    launches.push_back(L);
    done += L.n_frames;
    fb += L.n_frames;
  }
  for (const Launch& L : launches) {
    const std::vector<uint32_t> tab(tabs.begin() + (long)L.table, tabs.begin() + (long)L.table + 2 * (L.n_chunks + 1));
    if ((rc = EnqueueLaunch(t, s, L, tab, p)) != RT2_OK) return rc;
  }
  return RT2_OK;
}

}  // namespace

int rt2::detail::Flush(rt2_tracer* t) {
  if (t->queued == 0) return RT2_OK;
  const int n = t->queued;
  t->queued = 0;
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = LaunchFrames(t, n);
  t->enqueue_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}


extern "C" {

// Update()/Render() only queue frames: the queued frames are launched together when a result is
// read (any readback, query, synchronize, stats), when a setting that affects them changes, or
// when lazy_max frames are queued. Results cannot tell the difference (samples are summed in frame
// order), but App::Run's headless pattern — num_samples x Update() then one readback
// (App.cpp:243-248) — then runs as one launch instead of num_samples one-frame launches, each
// of which would be as long as its longest path.
int rt2_tracer_render(rt2_tracer* t, int n_frames) {
  if (!t || n_frames < 0) return Fail(RT2_ERR_INVALID, "n_frames must be >= 0");
  RT2_FORWARD(t, rt2_tracer_render(p, n_frames));
  if ((int64_t)t->frame_idx + t->queued + n_frames > 0x7FFFFFFF)
    return Fail(RT2_ERR_INVALID, "frame index overflow");
  if (t->camera.Params().sqrt_spp <= 0) return Fail(RT2_ERR_INVALID, "samples_per_pixel gives sqrt_spp = 0");
  if (t->origins_bounded && !CameraOriginsBounded(t->camera.Params())) return Fail(RT2_ERR_INVALID, kCameraRangeMsg);
  t->queued += n_frames;
  if (t->lazy_max > 0 && t->queued < t->lazy_max) return RT2_OK;
  return Flush(t);
}

int rt2_tracer_set_lazy_frames(rt2_tracer* t, int max_queued) {
  if (!t || max_queued < 0) return Fail(RT2_ERR_INVALID, "max_queued must be >= 0");
  RT2_FORWARD(t, rt2_tracer_set_lazy_frames(p, max_queued));
  t->lazy_max = max_queued;
  if (max_queued == 0 || t->queued >= max_queued) return Flush(t);
  return RT2_OK;
}

int rt2_tracer_update(rt2_tracer* t) { return rt2_tracer_render(t, 1); }

int rt2_tracer_flush(rt2_tracer* t) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  RT2_FORWARD(t, rt2_tracer_flush(p));
  return Flush(t);
}

int rt2_tracer_synchronize(rt2_tracer* t) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  RT2_FORWARD(t, rt2_tracer_synchronize(p));
  return Sync(t);
}

int64_t rt2_tracer_frame_idx(const rt2_tracer* t) {
  if (!t) return -1;
  if (IsMulti(t)) return rt2_tracer_frame_idx(t->parts[0]);
  return t->frame_idx + t->queued;
}

int rt2_tracer_dims(const rt2_tracer* t, int* w, int* h) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  if (w) *w = t->width;
  if (h) *h = t->height;
  return RT2_OK;
}

int rt2_tracer_local_rows(const rt2_tracer* t) {
  if (!t) return -1;
  return IsMulti(t) ? t->height : t->local_rows;
}

int rt2_tracer_n_gpus(const rt2_tracer* t) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  return IsMulti(t) ? (int)t->parts.size() : 1;
}

int rt2_tracer_accumulation(rt2_tracer* t, float* out) {
  if (!t || !out) return Fail(RT2_ERR_INVALID, "null argument");
  if (IsMulti(t)) {
    int rc = GatherMulti(t);
    return rc != RT2_OK ? rc : rt2_tracer_image_accumulation(t, out);
  }
  int rc = Sync(t);
  if (rc != RT2_OK) return rc;
  size_t n = (size_t)t->width * (size_t)t->local_rows;
  if (n) HIP_TRY(hipMemcpy(out, t->d_accum.get<float>(), n * 3 * sizeof(float), hipMemcpyDeviceToHost));
  return RT2_OK;
}

int rt2_tracer_non_converted_pixels(rt2_tracer* t, float* out) {
  if (t && out && IsMulti(t) && t->parts[0]->image_adaptive) {
    // adaptive sampling of the gathered image: the counts travelled with the gather and the root's kernel divided
    // each pixel's sum by its own (the same IEEE quotient as the host's below)
    int rc = GatherMulti(t);
    return rc != RT2_OK ? rc : rt2_tracer_image_non_converted_pixels(t, out);
  }
  int rc = rt2_tracer_accumulation(t, out);
  if (rc != RT2_OK) return rc;
  size_t n = (size_t)t->width * (size_t)rt2_tracer_local_rows(t) * 3;
  if (t->adaptive_on) {  // adaptive sampling: each pixel's sum over its own sample count
    std::vector<uint32_t> np(n / 3);
    if ((rc = SampleCountsLocal(t, np.data())) != RT2_OK) return rc;
    for (size_t i = 0; i < n; i++) out[i] = out[i] / (float)np[i / 3];
    return RT2_OK;
  }
  float f = (float)rt2_tracer_frame_idx(t);  // accumulation / frame_idx_ (RayTracer.cpp:108-109)
  for (size_t i = 0; i < n; i++) out[i] = out[i] / f;
  return RT2_OK;
}

int rt2_tracer_pixels(rt2_tracer* t, uint8_t* out) {
  if (!t || !out) return Fail(RT2_ERR_INVALID, "null argument");
  if (IsMulti(t)) {
    int rc = GatherMulti(t);
    return rc != RT2_OK ? rc : rt2_tracer_image_pixels(t, out);
  }
  int rc = Sync(t);
  if (rc != RT2_OK) return rc;
  size_t n = (size_t)t->width * (size_t)t->local_rows;
  if (n) HIP_TRY(hipMemcpy(out, t->d_pixels.get<uint8_t>(), n * 4, hipMemcpyDeviceToHost));
  return RT2_OK;
}

int rt2_tracer_pixels_async(rt2_tracer* t, uint8_t* out) {
  if (!t || !out) return Fail(RT2_ERR_INVALID, "null argument");
  if (IsMulti(t)) {
    int rc = GatherMulti(t);
    if (rc != RT2_OK) return rc;
    rt2_tracer* r = t->parts[0];
    HIP_TRY(hipSetDevice(r->device));
    size_t n = (size_t)t->width * (size_t)t->height;
    if (n) HIP_TRY(hipMemcpyAsync(out, r->d_image_px.get<uint8_t>(), n * 4, hipMemcpyDeviceToHost, r->stream));
    return RT2_OK;
  }
  int rc = Flush(t);
  if (rc != RT2_OK) return rc;
  HIP_TRY(hipSetDevice(t->device));
  size_t n = (size_t)t->width * (size_t)t->local_rows;
  if (n) HIP_TRY(hipMemcpyAsync(out, t->d_pixels.get<uint8_t>(), n * 4, hipMemcpyDeviceToHost, t->stream));
  return RT2_OK;
}

int rt2_tracer_query(rt2_tracer* t) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  if (IsMulti(t)) {
    int all = 1;
    for (rt2_tracer* p : t->parts) {
      int q = rt2_tracer_query(p);
      if (q < 0) return q;
      all &= q;
    }
    return all;
  }
  int rc = Flush(t);
  if (rc != RT2_OK) return rc;
  HIP_TRY(hipSetDevice(t->device));
  hipError_t e = hipStreamQuery(t->stream);
  if (e == hipSuccess) return 1;
  if (e == hipErrorNotReady) return 0;
  return HipFail(e, "hipStreamQuery");
}

int rt2_host_alloc(size_t bytes, void** out) {
  if (!out) return Fail(RT2_ERR_INVALID, "null argument");
  *out = nullptr;
  HIP_TRY(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
  return RT2_OK;
}

void rt2_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

int rt2_tracer_copy_accum_device(rt2_tracer* t, void* dst, void* stream) {
  if (!t || !dst) return Fail(RT2_ERR_INVALID, "null argument");
  const float* src;
  size_t n;
  rt2_tracer* o = t;  // the tracer whose stream orders the copy
  if (IsMulti(t)) {
    int rc = GatherMulti(t);
    if (rc != RT2_OK) return rc;
    o = t->parts[0];
    src = o->d_image.get<float>();
    n = (size_t)t->width * (size_t)t->height;
  } else {
    int rc = Flush(t);
    if (rc != RT2_OK) return rc;
    src = t->d_accum.get<float>();
    n = (size_t)t->width * (size_t)t->local_rows;
  }
  HIP_TRY(hipSetDevice(o->device));
  hipStream_t s = stream ? (hipStream_t)stream : o->stream;
  if (s != o->stream) {
    hipEvent_t e = TakeEvent(o);
    if (!e) return Fail(RT2_ERR_HIP, "event create failed");
    HIP_TRY(hipEventRecord(e, o->stream));
    HIP_TRY(hipStreamWaitEvent(s, e, 0));
    o->event_pool.push_back(e);
  }
  if (n) HIP_TRY(hipMemcpyAsync(dst, src, n * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
  return RT2_OK;
}

int rt2_tracer_enable_ray_counts(rt2_tracer* t, int on) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  RT2_FORWARD(t, rt2_tracer_enable_ray_counts(p, on));
  int rc = Sync(t);
  if (rc != RT2_OK) return rc;
  t->ray_counts_on = on != 0;
  if ((rc = Realloc(t)) != RT2_OK) return rc;
  return ResetFrame(t);
}

int rt2_tracer_ray_counts(rt2_tracer* t, uint32_t* out) {
  if (!t || !out) return Fail(RT2_ERR_INVALID, "null argument");
  if (IsMulti(t))  // a diagnostic: each GPU's rows read back and placed on the host
    return PlacePartRows(t, out, 1, [](rt2_tracer* p, uint32_t* rows) { return rt2_tracer_ray_counts(p, rows); });
  if (!t->d_ray_counts) return Fail(RT2_ERR_INVALID, "ray counts not enabled");
  int rc = Sync(t);
  if (rc != RT2_OK) return rc;
  size_t n = (size_t)t->width * (size_t)t->local_rows;
  if (n) HIP_TRY(hipMemcpy(out, t->d_ray_counts.get<uint32_t>(), n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RT2_OK;
}

int rt2_tracer_enable_stats(rt2_tracer* t, int on) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  RT2_FORWARD(t, rt2_tracer_enable_stats(p, on));
  int rc = FlushIfChanged(t, t->stats_on, on != 0);
  if (rc != RT2_OK) return rc;
  t->stats_on = on != 0;
  return RT2_OK;
}

int rt2_tracer_get_stats(rt2_tracer* t, rt2_stats* o) {
  if (!t || !o) return Fail(RT2_ERR_INVALID, "null argument");
  if (IsMulti(t)) {  // sums over the GPUs; launches per GPU, kernel_ms of the busiest GPU
    rt2_stats sum;
    memset(&sum, 0, sizeof(sum));
    for (rt2_tracer* p : t->parts) {
      rt2_stats s;
      int rc = rt2_tracer_get_stats(p, &s);
      if (rc != RT2_OK) return rc;
      sum.rays += s.rays;
      sum.paths += s.paths;
      sum.bvh_tests += s.bvh_tests;
      sum.quad_tests += s.quad_tests;
      sum.sphere_tests += s.sphere_tests;
      sum.xform_visits += s.xform_visits;
      sum.medium_tests += s.medium_tests;
      sum.list_visits += s.list_visits;
      sum.overflow += s.overflow;
      sum.box_tests += s.box_tests;
      sum.box_certified += s.box_certified;
      sum.box_wave_visits += s.box_wave_visits;
      sum.box_wave_runs += s.box_wave_runs;
      sum.flat_uncertified += s.flat_uncertified;
      sum.flat_wave_fallbacks += s.flat_wave_fallbacks;
      sum.flat_fallback_hits += s.flat_fallback_hits;
      sum.hit_table_bytes = std::max(sum.hit_table_bytes, s.hit_table_bytes);
      sum.launches = std::max(sum.launches, s.launches);
      sum.kernel_ms = std::max(sum.kernel_ms, s.kernel_ms);
      sum.launch_ms_sum = std::max(sum.launch_ms_sum, s.launch_ms_sum);
      for (int k = 0; k < 4; k++) sum.stamps[k] += s.stamps[k];
      for (int k = 0; k < 8; k++) sum.diag[k] += s.diag[k];
      sum.gathers += s.gathers;
      sum.gather_ms += s.gather_ms;
      sum.enqueue_ms += s.enqueue_ms;
      sum.readbacks += s.readbacks;
      sum.readback_ms += s.readback_ms;
      sum.host_waits += s.host_waits;
      sum.sample_buffer_bytes = std::max(sum.sample_buffer_bytes, s.sample_buffer_bytes);
      sum.device_bytes_peak = std::max(sum.device_bytes_peak, s.device_bytes_peak);
    }
    *o = sum;
    return RT2_OK;
  }
  const uint64_t waits = t->host_waits;  // (this diagnostic's own synchronization is not counted)
  int rc = Sync(t);
  t->host_waits = waits;
  if (rc != RT2_OK) return rc;
  unsigned long long s[kStatsSlots];
  HIP_TRY(hipSetDevice(t->device));
  HIP_TRY(hipMemcpy(s, t->d_stats.get<unsigned long long>(), sizeof(s), hipMemcpyDeviceToHost));
  o->rays = s[StatsCounters::kRays];
  o->paths = t->paths;  // every (pixel, frame) of a launch finishes exactly one camera path
  o->bvh_tests = s[StatsCounters::kBvhTests];
  o->quad_tests = s[StatsCounters::kQuadTests];
  o->sphere_tests = s[StatsCounters::kSphereTests];
  o->xform_visits = s[StatsCounters::kXformVisits];
  o->medium_tests = s[StatsCounters::kMediumTests];
  o->list_visits = s[StatsCounters::kListVisits];
  o->overflow = s[StatsCounters::kCount];
  o->box_tests = s[StatsCounters::kBoxTests];
  o->box_certified = s[StatsCounters::kBoxCertified];
  o->box_wave_visits = s[StatsCounters::kBoxWaveVisits];
  o->box_wave_runs = s[StatsCounters::kBoxWaveRuns];
  o->flat_uncertified = s[StatsCounters::kFlatUncertified];
  o->flat_wave_fallbacks = s[StatsCounters::kFlatWaveFallbacks];
  o->flat_fallback_hits = s[StatsCounters::kFlatFallbackHits];
  o->hit_table_bytes = t->last_hit_bytes;
  for (int k = 0; k < 4; k++) o->stamps[k] = s[StatsCounters::kStamps + k];
  for (int k = 0; k < 8; k++) o->diag[k] = s[StatsCounters::kDiag + k];
  o->launches = t->launches;
  o->kernel_ms = t->kernel_ms;
  o->launch_ms_sum = t->launch_ms_sum;
  o->gathers = t->gathers;
  o->gather_ms = t->gather_ms;
  o->enqueue_ms = t->enqueue_ms;
  o->readbacks = t->readbacks;
  o->readback_ms = t->readback_ms;
  o->host_waits = t->host_waits;
  o->sample_buffer_bytes = t->slots[0].samples.bytes() + t->slots[1].samples.bytes();
  o->device_bytes_peak = std::max(t->device_bytes_peak, DeviceBytes(t));
  return RT2_OK;
}

int rt2_tracer_part_stats(rt2_tracer* t, int part, rt2_stats* o) {
  if (!t || !o) return Fail(RT2_ERR_INVALID, "null argument");
  const int n = IsMulti(t) ? (int)t->parts.size() : 1;
  if (part < 0 || part >= n) return Fail(RT2_ERR_INVALID, "rt2_tracer_part_stats: part out of range");
  return rt2_tracer_get_stats(IsMulti(t) ? t->parts[(size_t)part] : t, o);
}

int rt2_selftest(int device, int which, uint64_t n, uint64_t seed, uint64_t* mismatches, uint64_t* checked) {
  if (!mismatches || !checked) return Fail(RT2_ERR_INVALID, "null argument");
  if (which < 0 || which > 9) return Fail(RT2_ERR_INVALID, "unknown self-test");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return Fail(RT2_ERR_HIP, "no HIP device available");
  HIP_TRY(hipSetDevice(device));
  DeviceBuffer buf;
  HIP_TRY(buf.Alloc(2 * sizeof(unsigned long long)));
  unsigned long long* d = buf.get<unsigned long long>();
  unsigned long long h[2] = {0, 0};
  hipError_t e = hipMemset(d, 0, sizeof(h));
  if (e == hipSuccess) e = LaunchSelftest(which, (unsigned long long)n, (uint32_t)seed, d, nullptr);
  if (e == hipSuccess) e = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return HipFail(e, "self-test");
  *mismatches = h[0];
  *checked = h[1];
  return RT2_OK;
}

int rt2_tracer_reset_stats(rt2_tracer* t) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  RT2_FORWARD(t, rt2_tracer_reset_stats(p));
  int rc = Sync(t);
  if (rc != RT2_OK) return rc;
  HIP_TRY(hipSetDevice(t->device));
  HIP_TRY(hipMemset(t->d_stats.get<unsigned long long>(), 0, kStatsSlots * sizeof(unsigned long long)));
  t->launches = 0;
  t->paths = 0;
  t->kernel_ms = 0;
  t->launch_ms_sum = 0;
  t->busy_end = 0;
  t->gathers = 0;
  t->gather_ms = 0;
  t->enqueue_ms = 0;
  t->readbacks = 0;
  t->readback_ms = 0;
  t->host_waits = 0;
  return RT2_OK;
}

int rt2_band_rows_max(int height, int band_h, int world) {
  if (height < 0 || band_h < 0 || world < 1) return Fail(RT2_ERR_INVALID, "bad band layout");
  return rt2::BandRowsMax(height, band_h, world);
}

int rt2_deinterleave_host(const float* stacks, float* image, int width, int height, int band_h, int world,
                          int max_rows, int channels) {
  if (!stacks || !image || width < 0 || height < 0 || band_h < 0 || world < 1 || channels < 1)
    return Fail(RT2_ERR_INVALID, "bad de-interleave arguments");
  if (max_rows < rt2::BandRowsMax(height, band_h, world))
    return Fail(RT2_ERR_INVALID, "max_rows is below the largest rank's band stack");
  const size_t row = (size_t)width * (size_t)channels;
  for (int y = 0; y < height; y++) {
    const BandRow src = BandSource(y, band_h, world);
    memcpy(image + (size_t)y * row, stacks + ((size_t)src.rank * (size_t)max_rows + (size_t)src.row) * row,
           row * sizeof(float));
  }
  return RT2_OK;
}

int rt2_runtime_info(char* out, size_t cap) {
  if (!out || cap == 0) return Fail(RT2_ERR_INVALID, "null argument");
  int v = 0;
  (void)ncclGetVersion(&v);
  auto path_of = [](const void* sym) {
    Dl_info di;
    return dladdr(sym, &di) && di.dli_fname ? std::string(di.dli_fname) : std::string("?");
  };
  const std::string s = "rccl " + std::to_string(v) + " " + path_of((const void*)&ncclGetVersion) + "; hip " +
                        path_of((const void*)&hipGetDeviceCount);
  snprintf(out, cap, "%s", s.c_str());
  return RT2_OK;
}

int rt2_write_image(const float* pixels, int w, int h, const char* path, int png) {
  if (!pixels || !path || w <= 0 || h <= 0) return Fail(RT2_ERR_INVALID, "bad image arguments");
  std::string err;
  if (!WriteImage(pixels, w, h, path, png != 0, err)) return Fail(RT2_ERR_IO, err);
  return RT2_OK;
}

}  // extern "C"
