// Compile-and-link check of the ambient occlusion members of include/rt2/RayTracer.hpp: a point on the floor under
// the centre of the view from host memory, the image's counts, and both again from device memory without a wait.
#include <cfloat>
#include <cstdint>
#include <vector>

#include <rt2/RayTracer.hpp>

int FloorPoint(const char* scene_path, float* d_points, uint32_t* d_out) {
  rt2::serialize::SceneLoader loader;
  auto scene_opt = loader.LoadScene(scene_path);
  if (!scene_opt.has_value()) return 1;
  rt2::Scene& scene = scene_opt.value();
  rt2::RayTracer tracer(scene, 0);  // no OnResize: point mode needs no image
  const rt2::Camera& c = scene.cam;
  std::vector<float> points = {c.lookat_.x, 0.0f, c.lookat_.z, FLT_MAX, 0.0f, 1.0f, 0.0f, 0.0f};
  if (!rt2::RayTracer::RayValid(points.data())) return 2;
  std::vector<uint32_t> count(1, 0x55555555u);
  tracer.AmbientPoints(points.data(), 1, 16, count.data());
  const double ms = tracer.AmbientTime();
  tracer.AmbientPointsDevice(d_points, 1, 16, d_out, rt2::RayTracer::kDefaultSeed + 1);
  while (!tracer.Query()) {
  }
  tracer.OnResize({8, 8});
  std::vector<uint32_t> image(64, 0x55555555u);
  tracer.Ambient(16, 100.0f, image.data());
  tracer.AmbientDevice(16, FLT_MAX, d_out);
  tracer.Synchronize();
  return count[0] <= 16u && ms >= 0.0 && tracer.AmbientTime() >= 0.0 ? 0 : 3;
}

int main(int argc, char** argv) { return argc > 3 ? FloorPoint(argv[1], nullptr, nullptr) : 0; }
