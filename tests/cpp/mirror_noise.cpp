// Compile-only check of the noise members of include/rt2/RayTracer.hpp: render until the rms noise
// estimate meets a target, then read the estimate back.
#include <rt2/RayTracer.hpp>

int RenderUntilRun(const char* scene_path, const char* out_png, float target_rms, int max_samples) {
  rt2::serialize::SceneLoader loader;
  auto scene_opt = loader.LoadScene(scene_path);
  if (!scene_opt.has_value()) return 1;
  rt2::Scene& scene = scene_opt.value();
  rt2::RayTracer tracer(scene, 0);
  scene.cam.SetSamplesPerPixel(max_samples);
  tracer.camera = &scene.cam;
  tracer.OnResize(scene.dims);
  tracer.EnableMoments();
  const rt2_noise last = tracer.RenderUntil(scene, target_rms, max_samples, /*min_frames=*/32);
  const rt2_noise now = tracer.Noise(target_rms);
  const std::vector<rt2::vec3> sem = tracer.StandardError(), q = tracer.Moments();
  rt2::util::WriteImage(tracer.NonConvertedPixels(), tracer.Dims().x, tracer.Dims().y, out_png);
  return last.frames == now.frames && sem.size() == q.size() && last.rms <= target_rms ? 0 : 2;
}
