// rt2/RayTracer.hpp — header-only C++ mirror of the reference's hot-path interface over the C ABI
// (include/rt2.h), so reference callers (App::Run, src/App.cpp:81-249) switch by changing includes:
//
//   reference                                   here
//   raytrace2::cpu::RayTracer                   rt2::RayTracer          (RayTracer.hpp:15-42)
//   raytrace2::cpu::Scene (+ App.cpp:126 BVH)   rt2::Scene
//   raytrace2::cpu::Camera (scene.cam)          rt2::Camera (scene.cam, a value type)
//   serialize::SceneLoader::LoadScene           rt2::serialize::SceneLoader::LoadScene
//   serialize::LoadCamera / WriteCamera         rt2::serialize::LoadCamera / WriteCamera
//   serialize::LoadAppSettings                  rt2::serialize::LoadAppSettings
//   util::WriteImage                            rt2::util::WriteImage
//
// Differences a caller sees: the tracer renders on GPUs (device index, or a GPU count, at
// construction) and owns device buffers; Update() takes the scene only for signature compatibility
// (the scene program was uploaded at construction); errors throw rt2::Error (the C ABI itself never
// throws). With n_gpus > 1 the image is split into interleaved row bands over the GPUs and gathered
// over RCCL before every readback (rt2_tracer_create_multi); results are identical to one GPU.
#pragma once

#include <cstdint>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../rt2.h"

namespace rt2 {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

inline void Check(int rc) {
  if (rc < 0) throw Error(rc, rt2_last_error());
}

struct ivec2 {
  int x = 0, y = 0;
};
struct vec3 {
  float x = 0, y = 0, z = 0;
};
struct u8vec4 {
  uint8_t x = 0, y = 0, z = 0, w = 0;
};
using PixelArray = std::vector<u8vec4>;

// The camera fields the scene files carry (Camera.hpp:113-123); Update() happens on the device side.
struct Camera {
  vec3 center_{0, 0, 1}, lookat_{0, 0, 0}, view_up_{0, 1, 0};
  float vfov_ = 90.f, defocus_angle_ = 0, focus_dist_ = 1;
  int samples_per_pixel_ = 1;

  void SetCenter(const vec3& c) { center_ = c; }
  void SetLookAt(const vec3& c) { lookat_ = c; }
  void SetViewUp(const vec3& c) { view_up_ = c; }
  void SetFOV(float f) { vfov_ = f; }
  void SetDefocusAngle(float a) { defocus_angle_ = a; }
  void SetFocusDistance(float d) { focus_dist_ = d; }
  void SetSamplesPerPixel(int s) { samples_per_pixel_ = s; }
  [[nodiscard]] float GetFOV() const { return vfov_; }
  [[nodiscard]] int SamplesPerPixel() const { return samples_per_pixel_; }

  rt2_camera_desc Desc() const {
    rt2_camera_desc d{};
    d.center[0] = center_.x, d.center[1] = center_.y, d.center[2] = center_.z;
    d.look_at[0] = lookat_.x, d.look_at[1] = lookat_.y, d.look_at[2] = lookat_.z;
    d.view_up[0] = view_up_.x, d.view_up[1] = view_up_.y, d.view_up[2] = view_up_.z;
    d.vfov = vfov_, d.defocus_angle = defocus_angle_, d.focus_distance = focus_dist_;
    return d;
  }
  static Camera FromDesc(const rt2_camera_desc& d) {
    Camera c;
    c.center_ = {d.center[0], d.center[1], d.center[2]};
    c.lookat_ = {d.look_at[0], d.look_at[1], d.look_at[2]};
    c.view_up_ = {d.view_up[0], d.view_up[1], d.view_up[2]};
    c.vfov_ = d.vfov, c.defocus_angle_ = d.defocus_angle, c.focus_dist_ = d.focus_distance;
    return c;
  }
};

struct AppSettings {  // Settings.hpp:5-11
  bool render_once = false;
  bool save_after_render_once = false;
  size_t num_samples = 1;
  size_t max_depth = 50;
  bool render_window = true;
};

// A loaded scene: materials, textures, object graph with the top-level BVH (App.cpp:126).
class Scene {
 public:
  explicit Scene(rt2_scene* h) : h_(h, &rt2_scene_free) {
    rt2_camera_desc d{};
    Check(rt2_scene_get_camera(h, &d));
    cam = Camera::FromDesc(d);
    rt2_scene_info info{};
    Check(rt2_scene_get_info(h, &info));
    dims = {info.dims_x, info.dims_y};
    background_color = {info.background[0], info.background[1], info.background[2]};
  }
  rt2_scene* handle() const { return h_.get(); }

  Camera cam;
  ivec2 dims;
  vec3 background_color{1, 1, 1};

 private:
  std::shared_ptr<rt2_scene> h_;
};

namespace serialize {

struct SceneLoader {
  uint64_t seed = 0x5EED2024ull;
  std::string error;
  // Serialize.hpp:22 — std::nullopt on a schema error (message in `error`)
  [[nodiscard]] std::optional<Scene> LoadScene(const std::string& filepath) {
    rt2_scene* h = nullptr;
    if (rt2_scene_load(filepath.c_str(), seed, &h) != RT2_OK) {
      error = rt2_last_error();
      return std::nullopt;
    }
    return Scene(h);
  }
};

inline Camera LoadCamera(const std::string& filepath) {
  rt2_camera_desc d{};
  Check(rt2_camera_load(filepath.c_str(), &d));
  return Camera::FromDesc(d);
}

inline void WriteCamera(const Camera& cam, const std::string& filepath) {
  rt2_camera_desc d = cam.Desc();
  Check(rt2_camera_write(&d, filepath.c_str()));
}

inline AppSettings LoadAppSettings(const std::string& filepath) {
  rt2_app_settings s{};
  Check(rt2_settings_load(filepath.c_str(), &s));
  AppSettings a;
  a.render_once = s.render_once != 0;
  a.save_after_render_once = s.save_after_render_once != 0;
  a.num_samples = (size_t)s.num_samples;
  a.max_depth = (size_t)s.max_depth;
  a.render_window = s.render_window != 0;
  return a;
}

}  // namespace serialize

namespace util {
inline void WriteImage(const std::vector<vec3>& pixels, int width, int height, const std::string& out_path,
                       bool png = true) {
  Check(rt2_write_image(reinterpret_cast<const float*>(pixels.data()), width, height, out_path.c_str(), png ? 1 : 0));
}
}  // namespace util

// cpu::RayTracer (RayTracer.hpp:15-42) on MI355X GPUs: one GPU (`device`; n_gpus 0), or `n_gpus`
// GPUs starting at `device` with an RCCL gather of their row bands (band_h 0 = 2 rows; n_gpus 1
// is the same path with a communicator of size 1).
class RayTracer {
 public:
  explicit RayTracer(const Scene& scene, int device = 0, int n_gpus = 0, int band_h = 0) {
    rt2_tracer* t = nullptr;
    if (n_gpus <= 0) {
      Check(rt2_tracer_create(scene.handle(), device, &t));
    } else {
      std::vector<int> devs((size_t)n_gpus);
      for (int i = 0; i < n_gpus; i++) devs[(size_t)i] = device + i;
      Check(rt2_tracer_create_multi(scene.handle(), n_gpus, devs.data(), band_h, &t));
    }
    t_.reset(t);
  }

  void Update(const Scene& /*scene*/) {  // one frame (RayTracer.cpp:55-70)
    Sync();
    Check(rt2_tracer_update(t_.get()));
  }
  void Render(const Scene& /*scene*/, int n_frames) {  // n x Update in one launch
    Sync();
    Check(rt2_tracer_render(t_.get(), n_frames));
  }
  void OnResize(ivec2 dims) {  // RayTracer.cpp:87-104 (includes Reset)
    dims_ = dims;
    Check(rt2_tracer_on_resize(t_.get(), dims.x, dims.y));
  }
  void Reset() { Check(rt2_tracer_reset(t_.get())); }

  [[nodiscard]] std::vector<vec3> NonConvertedPixels() const {
    std::vector<vec3> out((size_t)dims_.x * LocalRows());
    Check(rt2_tracer_non_converted_pixels(t_.get(), reinterpret_cast<float*>(out.data())));
    return out;
  }
  [[nodiscard]] const PixelArray& Pixels() const {
    pixels_.resize((size_t)dims_.x * LocalRows());
    Check(rt2_tracer_pixels(t_.get(), reinterpret_cast<uint8_t*>(pixels_.data())));
    return pixels_;
  }
  [[nodiscard]] size_t FrameIdx() const { return (size_t)rt2_tracer_frame_idx(t_.get()); }
  [[nodiscard]] ivec2 Dims() const { return dims_; }
  bool OnEvent(const void* /*sdl_event*/) { return false; }  // no window on the GPU path
  void OnImGui() {}

  // Like the reference (RayTracer.hpp:31-32): `camera` points at scene.cam and is read at every
  // Update (camera->Update(), RayTracer.cpp:56), so moving it between Update() calls takes effect
  // at the next frame; max_depth likewise.
  Camera* camera = nullptr;
  size_t max_depth = 50;

  // Noise estimate (rt2.h "Noise estimate and render-until-converged"): sums of the samples' squares
  // beside the accumulation, the standard error per pixel, the image's noise scalars, and rendering
  // until the rms noise is at most a target. EnableMoments resets the frame like OnResize.
  void EnableMoments(bool on = true) { Check(rt2_tracer_enable_moments(t_.get(), on ? 1 : 0)); }
  [[nodiscard]] std::vector<vec3> Moments() const {
    std::vector<vec3> out((size_t)dims_.x * LocalRows());
    Check(rt2_tracer_moments(t_.get(), reinterpret_cast<float*>(out.data())));
    return out;
  }
  [[nodiscard]] std::vector<vec3> StandardError() const {
    std::vector<vec3> out((size_t)dims_.x * LocalRows());
    Check(rt2_tracer_standard_error(t_.get(), reinterpret_cast<float*>(out.data())));
    return out;
  }
  [[nodiscard]] rt2_noise Noise(float threshold = 0.f) const {
    rt2_noise n{};
    Check(rt2_tracer_noise(t_.get(), threshold, &n));
    return n;
  }
  rt2_noise RenderUntil(const Scene& /*scene*/, float target_rms, int max_frames, int min_frames = 0,
                        int check_every = 0) {
    Sync();
    rt2_noise n{};
    Check(rt2_tracer_render_until(t_.get(), target_rms, min_frames, max_frames, check_every, &n));
    return n;
  }

  // Adaptive sampling (rt2.h "Adaptive sampling"): converged pixels retire at a check and later launches
  // trace only the rest. Needs EnableMoments; EnableAdaptive resets the frame like OnResize.
  void EnableAdaptive(bool on = true) { Check(rt2_tracer_enable_adaptive(t_.get(), on ? 1 : 0)); }
  [[nodiscard]] std::vector<uint32_t> SampleCounts() const {
    std::vector<uint32_t> out((size_t)dims_.x * LocalRows());
    Check(rt2_tracer_sample_counts(t_.get(), out.data()));
    return out;
  }
  rt2_adaptive AdaptiveCheck(float threshold, int window = 1) {
    rt2_adaptive a{};
    Check(rt2_tracer_adaptive_check(t_.get(), threshold, window, &a));
    return a;
  }
  rt2_adaptive RenderAdaptive(const Scene& /*scene*/, float threshold, int max_frames, int window = 1,
                              int min_frames = 0, int check_every = 0) {
    Sync();
    rt2_adaptive a{};
    Check(rt2_tracer_render_adaptive(t_.get(), threshold, window, min_frames, max_frames, check_every, &a));
    return a;
  }

  // Feature buffers and denoiser (rt2.h "Feature buffers and denoiser"). Features: the first-hit record of
  // the ray through each local pixel's centre, 16 floats per pixel. Denoise: the variance-guided a-trous
  // filter over the mean image (needs EnableMoments, FrameIdx() >= 2, one unpartitioned GPU); params null:
  // the defaults (DenoiseDefaults); variance: receives the filtered variance of the mean when not null.
  static rt2_denoise_params DenoiseDefaults() {
    rt2_denoise_params p{};
    rt2_denoise_defaults(&p);
    return p;
  }
  [[nodiscard]] std::vector<float> Features() {
    Sync();
    std::vector<float> out((size_t)dims_.x * LocalRows() * 16);
    Check(rt2_tracer_features(t_.get(), out.data()));
    return out;
  }
  [[nodiscard]] std::vector<vec3> Denoise(const rt2_denoise_params* params = nullptr, std::vector<float>* variance = nullptr) {
    Sync();
    std::vector<vec3> out((size_t)dims_.x * LocalRows());
    if (variance) variance->assign(out.size(), 0.0f);
    Check(rt2_tracer_denoise(t_.get(), params, reinterpret_cast<float*>(out.data()), variance ? variance->data() : nullptr));
    return out;
  }

  // Temporal reuse (rt2.h "Temporal reuse"). TemporalPush right before the camera moves and Reset();
  // TemporalResolve then returns the current estimate blended with the reprojected history (needs what
  // Denoise needs), filtered by Denoise's filter when denoise is set; it changes nothing. params null: the
  // defaults (TemporalDefaults); variance / length: receive the variance of the mean and the length in
  // frames when not null.
  static rt2_temporal_params TemporalDefaults() {
    rt2_temporal_params p{};
    rt2_temporal_defaults(&p);
    return p;
  }
  [[nodiscard]] std::vector<vec3> TemporalResolve(const rt2_temporal_params* params = nullptr, bool denoise = false,
                                                  const rt2_denoise_params* denoise_params = nullptr,
                                                  std::vector<float>* variance = nullptr,
                                                  std::vector<float>* length = nullptr) {
    Sync();
    std::vector<vec3> out((size_t)dims_.x * LocalRows());
    if (variance) variance->assign(out.size(), 0.0f);
    if (length) length->assign(out.size(), 0.0f);
    Check(rt2_tracer_temporal_resolve(t_.get(), params, denoise ? 1 : 0, denoise_params, reinterpret_cast<float*>(out.data()),
                                      variance ? variance->data() : nullptr, length ? length->data() : nullptr));
    return out;
  }
  void TemporalPush(const rt2_temporal_params* params = nullptr) {
    Sync();
    Check(rt2_tracer_temporal_push(t_.get(), params));
  }
  void TemporalClear() { Check(rt2_tracer_temporal_clear(t_.get())); }

  // Presenting reconstructed frames (rt2.h "Presenting reconstructed frames"): the display path of the
  // reconstruction. PresentAsync enqueues blend, filter, tone map and the copy of Dims().x * LocalRows RGBA8
  // pixels into `out` (pinned memory from rt2_host_alloc makes it a DMA) and returns at once; the bytes are
  // complete once Query() returns true or after Synchronize(). Present is the blocking form. MoveCamera is
  // TemporalPush, the camera change and Reset() in one call that does not wait; the history is taken under the
  // camera of the last Update(), and `*camera`, when set, takes `to`'s fields (`to` may be `*camera` itself,
  // moved in place since that Update). params null: the defaults (PresentDefaults).
  static rt2_present_params PresentDefaults() {
    rt2_present_params p{};
    rt2_present_defaults(&p);
    return p;
  }
  void PresentAsync(u8vec4* out, const rt2_present_params* params = nullptr) {
    Sync();
    Check(rt2_tracer_present_async(t_.get(), params, reinterpret_cast<uint8_t*>(out)));
  }
  [[nodiscard]] const PixelArray& Present(const rt2_present_params* params = nullptr) {
    Sync();
    pixels_.resize((size_t)dims_.x * LocalRows());
    Check(rt2_tracer_present(t_.get(), params, reinterpret_cast<uint8_t*>(pixels_.data())));
    return pixels_;
  }
  void MoveCamera(const Camera& to, const rt2_temporal_params* params = nullptr) {
    const rt2_camera_desc d = to.Desc();
    Check(rt2_tracer_move_camera(t_.get(), &d, params));
    if (camera && camera != &to) {
      const int spp = camera->samples_per_pixel_;
      *camera = to;
      camera->samples_per_pixel_ = spp;
    }
  }
  [[nodiscard]] double PresentTime() {  // GPU ms of the last present's kernels; -1: not finished, or none
    double ms = -1.0;
    Check(rt2_tracer_present_time(t_.get(), &ms));
    return ms;
  }
  // Reconstructing the gathered image (rt2.h "Reconstructing the gathered image"): the three groups above for a
  // tracer over several GPUs (n_gpus >= 1) or a joined one, where the members above are refused; vectors hold the
  // whole image, Dims().x * Dims().y pixels, on rank 0. GatherEstimate gathers the sums and the sums of squares
  // (needs EnableMoments, FrameIdx() >= 2) and does not wait; ImageResolve, ImagePresent* and ImageMoveCamera run
  // it themselves when the estimate held is not the current frame's (a joined tracer must have called it).
  // ImageResolve is TemporalResolve and Denoise in one (params null: both stages on, at their defaults).
  void GatherEstimate() {
    Sync();
    Check(rt2_tracer_gather_estimate(t_.get()));
  }
  [[nodiscard]] std::vector<float> ImageVariance() {
    std::vector<float> out(ImagePixels());
    Check(rt2_tracer_image_variance(t_.get(), out.data()));
    return out;
  }
  [[nodiscard]] std::vector<float> ImageFeatures() {
    Sync();
    std::vector<float> out(ImagePixels() * 16);
    Check(rt2_tracer_image_features(t_.get(), out.data()));
    return out;
  }
  [[nodiscard]] std::vector<vec3> ImageResolve(const rt2_present_params* params = nullptr,
                                               std::vector<float>* variance = nullptr,
                                               std::vector<float>* length = nullptr) {
    Sync();
    std::vector<vec3> out(ImagePixels());
    if (variance) variance->assign(out.size(), 0.0f);
    if (length) length->assign(out.size(), 0.0f);
    Check(rt2_tracer_image_resolve(t_.get(), params, reinterpret_cast<float*>(out.data()),
                                   variance ? variance->data() : nullptr, length ? length->data() : nullptr));
    return out;
  }
  void ImagePresentAsync(u8vec4* out, const rt2_present_params* params = nullptr) {
    Sync();
    Check(rt2_tracer_image_present_async(t_.get(), params, reinterpret_cast<uint8_t*>(out)));
  }
  [[nodiscard]] const PixelArray& ImagePresent(const rt2_present_params* params = nullptr) {
    Sync();
    pixels_.resize(ImagePixels());
    Check(rt2_tracer_image_present(t_.get(), params, reinterpret_cast<uint8_t*>(pixels_.data())));
    return pixels_;
  }
  void ImageMoveCamera(const Camera& to, const rt2_temporal_params* params = nullptr) {
    const rt2_camera_desc d = to.Desc();
    Check(rt2_tracer_image_move_camera(t_.get(), &d, params));
    if (camera && camera != &to) {
      const int spp = camera->samples_per_pixel_;
      *camera = to;
      camera->samples_per_pixel_ = spp;
    }
  }
  [[nodiscard]] double ImagePresentTime() {  // GPU ms of the last image present's kernels; -1: not finished, or none
    double ms = -1.0;
    Check(rt2_tracer_image_present_time(t_.get(), &ms));
    return ms;
  }
  // Adaptive sampling of the gathered image (rt2.h "Adaptive sampling of the gathered image"): EnableAdaptive,
  // AdaptiveCheck, RenderAdaptive and SampleCounts for a tracer over several GPUs (n_gpus >= 1) or a joined one,
  // where those members are refused. The checks of the GPUs overlap and their scalars are summed; every gather
  // carries each pixel's sample count, so the gathered image and its reconstruction rest on it. Needs
  // EnableMoments; ImageEnableAdaptive resets the frame like OnResize. ImageSampleCounts: the whole image, after a
  // gather (any readback of a multi-GPU tracer runs one; GatherEstimate is one).
  void ImageEnableAdaptive(bool on = true) { Check(rt2_tracer_image_enable_adaptive(t_.get(), on ? 1 : 0)); }
  rt2_adaptive ImageAdaptiveCheck(float threshold, int window = 1) {
    rt2_adaptive a{};
    Check(rt2_tracer_image_adaptive_check(t_.get(), threshold, window, &a));
    return a;
  }
  rt2_adaptive ImageRenderAdaptive(const Scene& /*scene*/, float threshold, int max_frames, int window = 1,
                                   int min_frames = 0, int check_every = 0) {
    Sync();
    rt2_adaptive a{};
    Check(rt2_tracer_image_render_adaptive(t_.get(), threshold, window, min_frames, max_frames, check_every, &a));
    return a;
  }
  [[nodiscard]] std::vector<uint32_t> ImageSampleCounts() const {
    std::vector<uint32_t> out(ImagePixels());
    Check(rt2_tracer_image_sample_counts(t_.get(), out.data()));
    return out;
  }
  // Ray queries (rt2.h "Ray queries"): the scene's closest hit for n rays of the caller, 8 floats each (ox oy oz
  // tmax dx dy dz time) -> 16 floats each in the feature record's layout (slot 0: 1 hit, 0 miss, -1 not traced,
  // RayValid). seed keys a ConstantMedium's draws (the default: the tracer's). Intersect: host buffers; it runs
  // the queued frames and blocks. IntersectDevice: device pointers on the tracer's GPU; it only enqueues and is
  // complete after Synchronize() or when Query() returns true. IntersectTime: GPU ms of the last call's kernels
  // (-1: not finished, or none); never waits.
  static constexpr uint64_t kDefaultSeed = 0x5EED2024ull;
  static bool RayValid(const float* ray8) { return rt2_query_ray_valid(ray8) == 1; }
  void Intersect(const float* rays, int64_t n, float* out, uint64_t seed = kDefaultSeed) {
    Check(rt2_tracer_intersect(t_.get(), n, rays, seed, out));
  }
  void IntersectDevice(const float* d_rays, int64_t n, float* d_out, uint64_t seed = kDefaultSeed) {
    Check(rt2_tracer_intersect_device(t_.get(), n, d_rays, seed, d_out));
  }
  // Occluded / OccludedDevice: one int8_t per ray, 1 occluded, 0 clear, -1 not traced: slot 0 of Intersect's
  // record for the same ray and seed, from a walk that ends at its first hit. Host and device entry as above.
  void Occluded(const float* rays, int64_t n, int8_t* out, uint64_t seed = kDefaultSeed) {
    Check(rt2_tracer_occluded(t_.get(), n, rays, seed, out));
  }
  void OccludedDevice(const float* d_rays, int64_t n, int8_t* d_out, uint64_t seed = kDefaultSeed) {
    Check(rt2_tracer_occluded_device(t_.get(), n, d_rays, seed, d_out));
  }
  [[nodiscard]] double IntersectTime() {
    double ms = -1.0;
    Check(rt2_tracer_intersect_time(t_.get(), &ms));
    return ms;
  }
  // Ambient occlusion (rt2.h "Ambient occlusion"): per point the number of `samples` cosine-weighted occlusion
  // rays that are blocked, one uint32_t each, 0xFFFFFFFF for a miss pixel or an invalid point. Ambient: the image's
  // first hits (the cached feature records) within `radius` (FLT_MAX: unbounded), one word per local pixel into a
  // host buffer; a readback. AmbientPoints: n caller records, 8 floats each (px py pz tmax nx ny nz time). The
  // Device forms take device pointers, only enqueue and are complete when Query() returns true. AmbientTime: GPU ms
  // of the last call's kernels (-1: not finished, or none); never waits.
  void Ambient(int samples, float radius, uint32_t* out, uint64_t seed = kDefaultSeed) {
    Check(rt2_tracer_ambient(t_.get(), samples, radius, seed, out));
  }
  void AmbientDevice(int samples, float radius, uint32_t* d_out, uint64_t seed = kDefaultSeed) {
    Check(rt2_tracer_ambient_device(t_.get(), samples, radius, seed, d_out));
  }
  void AmbientPoints(const float* points, int64_t n, int samples, uint32_t* out, uint64_t seed = kDefaultSeed) {
    Check(rt2_tracer_ambient_points(t_.get(), n, points, samples, seed, out));
  }
  void AmbientPointsDevice(const float* d_points, int64_t n, int samples, uint32_t* d_out,
                           uint64_t seed = kDefaultSeed) {
    Check(rt2_tracer_ambient_points_device(t_.get(), n, d_points, samples, seed, d_out));
  }
  [[nodiscard]] double AmbientTime() {
    double ms = -1.0;
    Check(rt2_tracer_ambient_time(t_.get(), &ms));
    return ms;
  }
  // Radiance queries (rt2.h "Radiance queries"): RayColorForward along n rays of the caller (8 floats each, as
  // Intersect's), summed over params.samples paths per ray: 3 floats per ray into out_sum (the caller divides) and,
  // where out_rays is not null, the rays cast (0xFFFFFFFF for an invalid ray, whose sum is 0). streams: two uint32_t
  // (pixel word, frame word) per ray, or null for (index, 0x40000000). Radiance: host buffers; it runs the queued
  // frames and blocks. RadianceDevice: device pointers; it only enqueues and is complete when Query() returns true.
  // RadianceTime: GPU ms of the last call's kernels (-1: not finished yet, or none); never waits.
  [[nodiscard]] static rt2_radiance_params RadianceDefaults() {
    rt2_radiance_params p;
    rt2_radiance_defaults(&p);
    return p;
  }
  void Radiance(const float* rays, int64_t n, float* out_sum, uint32_t* out_rays = nullptr,
                const rt2_radiance_params& params = RadianceDefaults(), const uint32_t* streams = nullptr,
                uint64_t seed = kDefaultSeed) {
    Check(rt2_tracer_radiance(t_.get(), n, rays, streams, &params, seed, out_sum, out_rays));
  }
  void RadianceDevice(const float* d_rays, int64_t n, float* d_out_sum, uint32_t* d_out_rays = nullptr,
                      const rt2_radiance_params& params = RadianceDefaults(), const uint32_t* d_streams = nullptr,
                      uint64_t seed = kDefaultSeed) {
    Check(rt2_tracer_radiance_device(t_.get(), n, d_rays, d_streams, &params, seed, d_out_sum, d_out_rays));
  }
  [[nodiscard]] double RadianceTime() {
    double ms = -1.0;
    Check(rt2_tracer_radiance_time(t_.get(), &ms));
    return ms;
  }
  [[nodiscard]] bool Query() {
    const int q = rt2_tracer_query(t_.get());
    Check(q);
    return q == 1;
  }
  void Synchronize() { Check(rt2_tracer_synchronize(t_.get())); }

  rt2_tracer* handle() const { return t_.get(); }
  [[nodiscard]] int NumGpus() const { return rt2_tracer_n_gpus(t_.get()); }

 private:
  struct Deleter {
    void operator()(rt2_tracer* t) const { rt2_tracer_destroy(t); }
  };
  void Sync() {
    Check(rt2_tracer_set_max_depth(t_.get(), (int)max_depth));
    if (camera) {
      Check(rt2_tracer_set_samples_per_pixel(t_.get(), camera->samples_per_pixel_));
      rt2_camera_desc d = camera->Desc();
      Check(rt2_tracer_set_camera(t_.get(), &d));
    }
  }
  std::unique_ptr<rt2_tracer, Deleter> t_;
  ivec2 dims_;
  mutable PixelArray pixels_;
  int LocalRows() const { return rt2_tracer_local_rows(t_.get()); }
  size_t ImagePixels() const { return (size_t)dims_.x * (size_t)dims_.y; }
};

}  // namespace rt2
