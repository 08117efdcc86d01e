// Compile-and-link check of the ray-query members of include/rt2/RayTracer.hpp: pick what the centre of the view
// hits and focus the camera on it, then a visibility test between two points, from host buffers; the same rays
// from device memory without a wait.
#include <cfloat>
#include <cmath>
#include <vector>

#include <rt2/RayTracer.hpp>

int FocusOnCentre(const char* scene_path, float* d_rays, float* d_out) {
  rt2::serialize::SceneLoader loader;
  auto scene_opt = loader.LoadScene(scene_path);
  if (!scene_opt.has_value()) return 1;
  rt2::Scene& scene = scene_opt.value();
  rt2::RayTracer tracer(scene, 0);  // no OnResize: a query needs no image
  const rt2::Camera& c = scene.cam;
  const float dx = c.lookat_.x - c.center_.x, dy = c.lookat_.y - c.center_.y, dz = c.lookat_.z - c.center_.z;
  // the centre of the view, and from there back to the camera, bounded by the distance between the two
  std::vector<float> rays = {c.center_.x, c.center_.y, c.center_.z, FLT_MAX, dx, dy, dz, 0.0f,
                             c.lookat_.x, c.lookat_.y, c.lookat_.z, 1.0f,    -dx, -dy, -dz, 0.0f};
  if (!rt2::RayTracer::RayValid(rays.data())) return 2;
  std::vector<float> out(2 * 16);
  tracer.Intersect(rays.data(), 2, out.data());
  if (out[0] == 1.0f) scene.cam.SetFocusDistance(out[13]);
  const bool visible = out[16] == 0.0f;  // nothing between the two points
  const double ms = tracer.IntersectTime();
  tracer.IntersectDevice(d_rays, 2, d_out, rt2::RayTracer::kDefaultSeed + 1);
  while (!tracer.Query()) {
  }
  return visible && ms >= 0.0 && tracer.IntersectTime() >= 0.0 ? 0 : 3;
}

int main(int argc, char** argv) { return argc > 3 ? FocusOnCentre(argv[1], nullptr, nullptr) : 0; }
