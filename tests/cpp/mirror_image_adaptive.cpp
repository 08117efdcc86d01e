// Compile-only check of the members of include/rt2/RayTracer.hpp for adaptive sampling of the gathered image: a
// tracer over several GPUs renders adaptively, runs one more check by hand, gathers, reads the image's sample
// counts and resolves the reconstruction, whose lengths are those counts.
#include <rt2/RayTracer.hpp>

int ImageAdaptiveRun(const char* scene_path, const char* out_png, float threshold, int max_samples, int gpus) {
  rt2::serialize::SceneLoader loader;
  auto scene_opt = loader.LoadScene(scene_path);
  if (!scene_opt.has_value()) return 1;
  rt2::Scene& scene = scene_opt.value();
  rt2::RayTracer tracer(scene, 0, gpus);
  scene.cam.SetSamplesPerPixel(max_samples);
  tracer.camera = &scene.cam;
  tracer.OnResize(scene.dims);
  tracer.EnableMoments();
  tracer.ImageEnableAdaptive();
  const rt2_adaptive last = tracer.ImageRenderAdaptive(scene, threshold, max_samples, /*window=*/1, /*min_frames=*/32);
  const rt2_adaptive now = tracer.ImageAdaptiveCheck(threshold, 2);
  tracer.GatherEstimate();
  const std::vector<uint32_t> counts = tracer.ImageSampleCounts();
  std::vector<float> var, len;
  const std::vector<rt2::vec3> resolved = tracer.ImageResolve(nullptr, &var, &len);
  rt2::util::WriteImage(tracer.NonConvertedPixels(), tracer.Dims().x, tracer.Dims().y, out_png);
  tracer.ImageEnableAdaptive(false);
  const bool sizes = counts.size() == now.pixels && resolved.size() == counts.size() && len.size() == counts.size();
  return last.frames == now.frames && sizes && now.active <= last.active ? 0 : 2;
}
