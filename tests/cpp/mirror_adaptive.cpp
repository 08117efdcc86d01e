// Compile-only check of the adaptive-sampling members of include/rt2/RayTracer.hpp: render adaptively,
// run one more check by hand, then read the sample counts back.
#include <rt2/RayTracer.hpp>

int RenderAdaptiveRun(const char* scene_path, const char* out_png, float threshold, int max_samples) {
  rt2::serialize::SceneLoader loader;
  auto scene_opt = loader.LoadScene(scene_path);
  if (!scene_opt.has_value()) return 1;
  rt2::Scene& scene = scene_opt.value();
  rt2::RayTracer tracer(scene, 0);
  scene.cam.SetSamplesPerPixel(max_samples);
  tracer.camera = &scene.cam;
  tracer.OnResize(scene.dims);
  tracer.EnableMoments();
  tracer.EnableAdaptive();
  const rt2_adaptive last = tracer.RenderAdaptive(scene, threshold, max_samples, /*window=*/1, /*min_frames=*/32);
  const rt2_adaptive now = tracer.AdaptiveCheck(threshold, 2);
  const std::vector<uint32_t> counts = tracer.SampleCounts();
  rt2::util::WriteImage(tracer.NonConvertedPixels(), tracer.Dims().x, tracer.Dims().y, out_png);
  tracer.EnableAdaptive(false);
  return last.frames == now.frames && counts.size() == now.pixels && now.active <= last.active ? 0 : 2;
}
