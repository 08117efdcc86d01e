// Compile-only check of the temporal-reuse members of include/rt2/RayTracer.hpp: render with moments on, push
// the history, move the camera, reset, render a few frames and resolve, plain and filtered.
#include <rt2/RayTracer.hpp>

int RenderMovingRun(const char* scene_path, const char* out_png, int samples) {
  rt2::serialize::SceneLoader loader;
  auto scene_opt = loader.LoadScene(scene_path);
  if (!scene_opt.has_value()) return 1;
  rt2::Scene& scene = scene_opt.value();
  rt2::RayTracer tracer(scene, 0);
  scene.cam.SetSamplesPerPixel(samples);
  tracer.camera = &scene.cam;
  tracer.OnResize(scene.dims);
  tracer.EnableMoments();
  for (int i = 0; i < samples; i++) tracer.Update(scene);
  tracer.TemporalPush();
  rt2_camera_desc d = scene.cam.Desc();
  d.center[0] += 10.0f;
  rt2_tracer_set_camera(tracer.handle(), &d);
  tracer.camera = nullptr;
  tracer.Reset();
  for (int i = 0; i < 4; i++) tracer.Update(scene);
  const std::vector<rt2::vec3> plain = tracer.TemporalResolve();
  rt2_temporal_params p = rt2::RayTracer::TemporalDefaults();
  p.max_history = 64.0f;
  rt2_denoise_params dp = rt2::RayTracer::DenoiseDefaults();
  dp.iterations = 3;
  std::vector<float> variance, length;
  const std::vector<rt2::vec3> filtered = tracer.TemporalResolve(&p, true, &dp, &variance, &length);
  tracer.TemporalClear();
  rt2::util::WriteImage(filtered, tracer.Dims().x, tracer.Dims().y, out_png);
  return plain.size() == filtered.size() && variance.size() == length.size() ? 0 : 2;
}
