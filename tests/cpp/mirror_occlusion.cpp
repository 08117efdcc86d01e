// Compile-and-link check of the occlusion members of include/rt2/RayTracer.hpp: a shadow ray from the centre of
// the view back to the camera and an unbounded one along the view, from host buffers; the same rays from device
// memory without a wait.
#include <cfloat>
#include <cstdint>
#include <vector>

#include <rt2/RayTracer.hpp>

int ShadowOfCentre(const char* scene_path, float* d_rays, int8_t* d_out) {
  rt2::serialize::SceneLoader loader;
  auto scene_opt = loader.LoadScene(scene_path);
  if (!scene_opt.has_value()) return 1;
  rt2::Scene& scene = scene_opt.value();
  rt2::RayTracer tracer(scene, 0);  // no OnResize: a query needs no image
  const rt2::Camera& c = scene.cam;
  const float dx = c.lookat_.x - c.center_.x, dy = c.lookat_.y - c.center_.y, dz = c.lookat_.z - c.center_.z;
  // along the view without a bound; from the centre of the view back to the camera over (0.001, 0.999)
  std::vector<float> rays = {c.center_.x, c.center_.y, c.center_.z, FLT_MAX, dx, dy, dz, 0.0f,
                             c.lookat_.x, c.lookat_.y, c.lookat_.z, 0.999f,  -dx, -dy, -dz, 0.0f};
  if (!rt2::RayTracer::RayValid(rays.data())) return 2;
  std::vector<int8_t> occ(2, 0x55);
  tracer.Occluded(rays.data(), 2, occ.data());
  const bool answered = (occ[0] == 0 || occ[0] == 1) && (occ[1] == 0 || occ[1] == 1);
  const double ms = tracer.IntersectTime();  // the last query of either kind
  tracer.OccludedDevice(d_rays, 2, d_out, rt2::RayTracer::kDefaultSeed + 1);
  while (!tracer.Query()) {
  }
  return answered && ms >= 0.0 && tracer.IntersectTime() >= 0.0 ? 0 : 3;
}

int main(int argc, char** argv) { return argc > 3 ? ShadowOfCentre(argv[1], nullptr, nullptr) : 0; }
