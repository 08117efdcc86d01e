// Compile-only check of the feature-buffer and denoiser members of include/rt2/RayTracer.hpp: render with
// moments on, read the features, denoise at the defaults and with parameters of the caller's.
#include <rt2/RayTracer.hpp>

int RenderDenoisedRun(const char* scene_path, const char* out_png, int samples) {
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
  const std::vector<float> features = tracer.Features();
  const std::vector<rt2::vec3> plain = tracer.Denoise();
  rt2_denoise_params p = rt2::RayTracer::DenoiseDefaults();
  p.iterations = 3;
  p.sigma_l = 2.0f;
  std::vector<float> variance;
  const std::vector<rt2::vec3> tuned = tracer.Denoise(&p, &variance);
  rt2::util::WriteImage(tuned, tracer.Dims().x, tracer.Dims().y, out_png);
  return features.size() == 16 * plain.size() && variance.size() == tuned.size() ? 0 : 2;
}
