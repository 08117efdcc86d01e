// Compile-only check of the presenting members of include/rt2/RayTracer.hpp: the windowed loop of App::Run
// without the window: render with moments on, present into pinned memory without waiting, move the camera
// keeping the history, present again.
#include <rt2/RayTracer.hpp>

int PresentMovingRun(const char* scene_path, int samples) {
  rt2::serialize::SceneLoader loader;
  auto scene_opt = loader.LoadScene(scene_path);
  if (!scene_opt.has_value()) return 1;
  rt2::Scene& scene = scene_opt.value();
  rt2::RayTracer tracer(scene, 0);
  scene.cam.SetSamplesPerPixel(samples);
  tracer.camera = &scene.cam;
  tracer.OnResize(scene.dims);
  tracer.EnableMoments();
  const size_t n = (size_t)tracer.Dims().x * (size_t)tracer.Dims().y;
  void* pinned = nullptr;
  rt2::Check(rt2_host_alloc(n * sizeof(rt2::u8vec4), &pinned));
  rt2::u8vec4* shown = static_cast<rt2::u8vec4*>(pinned);
  for (int i = 0; i < samples; i++) tracer.Update(scene);
  tracer.PresentAsync(shown);
  while (!tracer.Query()) {
  }
  const double ms = tracer.PresentTime();
  rt2::Camera moved = scene.cam;
  moved.SetCenter({scene.cam.center_.x + 10.0f, scene.cam.center_.y, scene.cam.center_.z});
  rt2_temporal_params tp = rt2::RayTracer::TemporalDefaults();
  tp.max_history = 64.0f;
  tracer.MoveCamera(moved, &tp);
  for (int i = 0; i < 4; i++) tracer.Update(scene);
  rt2_present_params p = rt2::RayTracer::PresentDefaults();
  p.dp.iterations = 3;
  tracer.PresentAsync(shown, &p);
  tracer.Synchronize();
  p.denoise = 0;
  const rt2::PixelArray& blocking = tracer.Present(&p);
  const int rc = blocking.size() == n && ms != 0.0 && shown[0].w == 255 ? 0 : 2;
  rt2_host_free(pinned);
  return rc;
}
