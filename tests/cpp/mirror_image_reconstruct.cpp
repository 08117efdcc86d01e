// Compile-only check of the gathered-image members of include/rt2/RayTracer.hpp: a tracer over several GPUs
// renders with moments on, gathers the estimate, reads its variance and features, resolves and presents the
// reconstruction, moves the camera keeping the root's history, and presents again.
#include <rt2/RayTracer.hpp>

int ImageReconstructRun(const char* scene_path, int samples, int gpus) {
  rt2::serialize::SceneLoader loader;
  auto scene_opt = loader.LoadScene(scene_path);
  if (!scene_opt.has_value()) return 1;
  rt2::Scene& scene = scene_opt.value();
  rt2::RayTracer tracer(scene, 0, gpus);
  scene.cam.SetSamplesPerPixel(samples);
  tracer.camera = &scene.cam;
  tracer.OnResize(scene.dims);
  tracer.EnableMoments();
  const size_t n = (size_t)tracer.Dims().x * (size_t)tracer.Dims().y;
  for (int i = 0; i < samples; i++) tracer.Update(scene);
  tracer.GatherEstimate();
  const std::vector<float> variance = tracer.ImageVariance();
  const std::vector<float> features = tracer.ImageFeatures();
  rt2_present_params p = rt2::RayTracer::PresentDefaults();
  p.temporal = 0;
  std::vector<float> var, len;
  const std::vector<rt2::vec3> filtered = tracer.ImageResolve(&p, &var, &len);
  const std::vector<rt2::vec3> defaults = tracer.ImageResolve();
  void* pinned = nullptr;
  rt2::Check(rt2_host_alloc(n * sizeof(rt2::u8vec4), &pinned));
  rt2::u8vec4* shown = static_cast<rt2::u8vec4*>(pinned);
  tracer.ImagePresentAsync(shown);
  while (!tracer.Query()) {
  }
  const double ms = tracer.ImagePresentTime();
  rt2::Camera moved = scene.cam;
  moved.SetCenter({scene.cam.center_.x + 10.0f, scene.cam.center_.y, scene.cam.center_.z});
  rt2_temporal_params tp = rt2::RayTracer::TemporalDefaults();
  tp.max_history = 64.0f;
  tracer.ImageMoveCamera(moved, &tp);
  for (int i = 0; i < 4; i++) tracer.Update(scene);
  tracer.ImagePresentAsync(shown, &p);
  tracer.Synchronize();
  const rt2::PixelArray& blocking = tracer.ImagePresent(&p);
  const bool sizes = variance.size() == n && features.size() == 16 * n && filtered.size() == n && defaults.size() == n &&
                     var.size() == n && len.size() == n && blocking.size() == n;
  const int rc = sizes && ms != 0.0 && shown[0].w == 255 ? 0 : 2;
  rt2_host_free(pinned);
  return rc;
}
