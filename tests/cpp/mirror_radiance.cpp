// Compile check of the radiance members of include/rt2/RayTracer.hpp: a ray from the camera towards its look-at point
// from host memory with and without stream words and counts, and again from device memory without a wait.
#include <cfloat>
#include <cstdint>
#include <vector>

#include <rt2/RayTracer.hpp>

int CentreRay(const char* scene_path, float* d_rays, uint32_t* d_streams, float* d_sum, uint32_t* d_cast) {
  rt2::serialize::SceneLoader loader;
  auto scene_opt = loader.LoadScene(scene_path);
  if (!scene_opt.has_value()) return 1;
  rt2::Scene& scene = scene_opt.value();
  rt2::RayTracer tracer(scene, 0);  // no OnResize: a radiance query needs no image
  const rt2::Camera& c = scene.cam;
  std::vector<float> ray = {c.center_.x, c.center_.y, c.center_.z, FLT_MAX,
                            c.lookat_.x - c.center_.x, c.lookat_.y - c.center_.y, c.lookat_.z - c.center_.z, 0.0f};
  if (!rt2::RayTracer::RayValid(ray.data())) return 2;
  float sum[3] = {0.0f, 0.0f, 0.0f};
  uint32_t cast = 0;
  tracer.Radiance(ray.data(), 1, sum);
  rt2_radiance_params p = rt2::RayTracer::RadianceDefaults();
  p.samples = 16, p.max_depth = 5, p.first_draw = 3;
  const uint32_t words[2] = {7u, 3u};
  tracer.Radiance(ray.data(), 1, sum, &cast, p, words, rt2::RayTracer::kDefaultSeed + 1);
  const double ms = tracer.RadianceTime();
  tracer.RadianceDevice(d_rays, 1, d_sum, d_cast, p, d_streams);
  while (!tracer.Query()) {
  }
  tracer.RadianceDevice(d_rays, 1, d_sum);
  tracer.Synchronize();
  return cast >= 16u && cast <= 16u * 5u && ms >= 0.0 && tracer.RadianceTime() >= 0.0 ? 0 : 3;
}

int main(int argc, char** argv) { return argc > 5 ? CentreRay(argv[1], nullptr, nullptr, nullptr, nullptr) : 0; }
