// headless.cpp — the reference's headless App::Run path (src/App.cpp:81-174, 243-248) written against
// the C++ mirror include/rt2/RayTracer.hpp: load the settings and the scene, num_samples x
// Update(), WriteImage(NonConvertedPixels()). It is the integration check of the C++ drop-in
// boundary (tests/test_gpu_headless.py runs it and compares its PNG with the Python path's).
//
//   rt2_headless <scene.json> <out.png> [--settings settings.json] [--samples N] [--size WxH] [--gpus N]
//                [--noise-target X [--max-samples N]] [--adaptive THRESHOLD [--window N] [--max-samples N]]
//                [--denoise [--denoise-iterations N]]
//
//   rt2_headless <scene.json> --pick X Y [--size W H]
// --pick X Y renders nothing and writes no image: it prints the hit record (rt2.h "Ray queries": 16 floats, the
// feature record's layout) of the ray through the centre of pixel (X, Y) of a W x H image (default: the
// scene's dims, else 1600x900) as one JSON line: the record RayTracer::Features holds for that pixel.
//
//   rt2_headless <scene.json> --radiance OX OY OZ DX DY DZ [--samples K]
// --radiance renders nothing and writes no image: it path-traces K samples (default 1) along the ray from (OX, OY,
// OZ) in the direction (DX, DY, DZ), taken as given, unbounded, at time 0 (rt2.h "Radiance queries": the default
// stream words and the tracer's depth) and prints the mean radiance, sum / K in float, and the rays cast as one JSON
// line.
//
//   rt2_headless <scene.json> <out.png> --ao SAMPLES [--ao-radius R] [--size WxH]
// --ao SAMPLES renders nothing: it writes the ambient-occlusion visibility of the image's first hits (rt2.h "Ambient
// occlusion": RayTracer::Ambient with SAMPLES samples within R, default unbounded) as a grey image, 1 - count /
// SAMPLES in float per pixel and 1 where the pixel's ray missed, through WriteImage as every other image.
// Without --settings the reference's Settings.hpp defaults apply (num_samples 1, max_depth 50);
// --samples / --size override num_samples and the output dims (App.cpp:115-124: scene dims, else
// 1600x900). --gpus N renders on GPUs 0..N-1 (row bands + RCCL gather, rt2_tracer_create_multi).
// --noise-target X renders until the image's rms noise estimate is at most X instead of a fixed count
// (RenderUntil with moments on, one check per stratum sweep), at most N = --max-samples frames (default:
// num_samples), with samples_per_pixel = N; it prints "frames <n> rms <x>" on stderr.
// --adaptive THRESHOLD renders with adaptive sampling (RenderAdaptive with moments on, one check per
// stratum sweep, --window N columns, default 1): pixels whose noise estimate is at most THRESHOLD retire,
// at most N = --max-samples frames (default: num_samples); it prints "frames <f> active <a> samples <s>".
// --denoise turns moments on and writes the denoised image (RayTracer::Denoise: the variance-guided a-trous
// filter at its defaults, --denoise-iterations N passes) where it wrote the plain one; it composes with
// --noise-target and --adaptive and needs at least 2 frames. With --gpus N it writes RayTracer::ImageResolve of
// the gathered image (temporal off, denoise on: the same filter over the gathered estimate, the same bytes).
// --gpus N --adaptive THRESHOLD takes the members for adaptive sampling of the gathered image (ImageEnableAdaptive,
// ImageRenderAdaptive: every GPU's check, the scalars summed, the sample counts gathered with the image) and prints
// the same line; the image is the one-GPU command's, byte for byte.
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <rt2/RayTracer.hpp>

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s <scene.json> <out.png> [--settings f] [--samples N] [--size WxH] [--gpus N] "
                         "[--noise-target X [--max-samples N]] [--adaptive THRESHOLD [--window N] [--max-samples N]] "
                         "[--denoise [--denoise-iterations N]] (--denoise with --gpus N filters the gathered image)\n"
                         "       %s <scene.json> <out.png> --ao SAMPLES [--ao-radius R] [--size WxH]\n"
                         "       %s <scene.json> --pick X Y [--size W H]\n"
                         "       %s <scene.json> --radiance OX OY OZ DX DY DZ [--samples K]\n",
                 argv[0], argv[0], argv[0], argv[0]);
    return 2;
  }
  // (--pick: no output image, the options start right after the scene)
  const bool no_image = !std::strncmp(argv[2], "--", 2);
  const std::string scene_path = argv[1], out_path = no_image ? "" : argv[2];
  rt2::AppSettings settings;
  long samples = -1;
  rt2::ivec2 size{0, 0};
  int gpus = 0;  // 0: the one-GPU tracer; N >= 1: rt2_tracer_create_multi over GPUs 0..N-1
  float noise_target = -1.f;  // >= 0: render until converged
  long max_samples = -1;
  float adaptive = -1.f;  // >= 0: adaptive sampling with this threshold
  int window = 1;
  bool denoise = false;
  int denoise_iterations = 0;  // 0: the default
  bool pick = false;
  rt2::ivec2 pick_at{0, 0};
  bool radiance = false;
  float radiance_ray[8] = {0.0f, 0.0f, 0.0f, FLT_MAX, 0.0f, 0.0f, 0.0f, 0.0f};
  int ao_samples = 0;  // > 0: write the ambient-occlusion visibility instead of a render
  float ao_radius = FLT_MAX;
  try {
    for (int i = no_image ? 2 : 3; i < argc; i += 2) {
      if (!std::strcmp(argv[i], "--denoise")) {  // a flag: no value follows
        denoise = true;
        i -= 1;
        continue;
      }
      if (i + 1 >= argc) break;
      if (!std::strcmp(argv[i], "--denoise-iterations")) {
        denoise_iterations = std::atoi(argv[i + 1]);
        if (denoise_iterations < 1 || denoise_iterations > 8) {
          std::fprintf(stderr, "--denoise-iterations needs an integer in [1, 8]\n");
          return 2;
        }
      } else if (!std::strcmp(argv[i], "--settings")) {
        settings = rt2::serialize::LoadAppSettings(argv[i + 1]);
      } else if (!std::strcmp(argv[i], "--samples")) {
        samples = std::atol(argv[i + 1]);
      } else if (!std::strcmp(argv[i], "--gpus")) {
        gpus = std::atoi(argv[i + 1]);
      } else if (!std::strcmp(argv[i], "--noise-target")) {
        noise_target = std::strtof(argv[i + 1], nullptr);
        if (!(noise_target >= 0.f)) return 2;
      } else if (!std::strcmp(argv[i], "--adaptive")) {
        adaptive = std::strtof(argv[i + 1], nullptr);
        if (!(adaptive >= 0.f)) return 2;
      } else if (!std::strcmp(argv[i], "--window")) {
        char* end = nullptr;
        const long v = std::strtol(argv[i + 1], &end, 10);
        if (end == argv[i + 1] || *end != '\0' || v < 0 || v > 64) {
          std::fprintf(stderr, "--window needs an integer in [0, 64]\n");
          return 2;
        }
        window = (int)v;
      } else if (!std::strcmp(argv[i], "--max-samples")) {
        max_samples = std::atol(argv[i + 1]);
      } else if (!std::strcmp(argv[i], "--ao")) {
        ao_samples = std::atoi(argv[i + 1]);
        if (ao_samples < 1 || ao_samples > 65535) {
          std::fprintf(stderr, "--ao needs an integer in [1, 65535]\n");
          return 2;
        }
      } else if (!std::strcmp(argv[i], "--ao-radius")) {
        ao_radius = std::strtof(argv[i + 1], nullptr);
        if (!(ao_radius > 0.001f) || std::isinf(ao_radius)) {
          std::fprintf(stderr, "--ao-radius needs a finite number above 0.001\n");
          return 2;
        }
      } else if (!std::strcmp(argv[i], "--pick")) {  // two values follow
        if (i + 2 >= argc || std::sscanf(argv[i + 1], "%d", &pick_at.x) != 1 || std::sscanf(argv[i + 2], "%d", &pick_at.y) != 1)
          return 2;
        pick = true;
        i += 1;
      } else if (!std::strcmp(argv[i], "--radiance")) {  // six values follow
        bool six = i + 6 < argc;
        for (int k = 0; six && k < 6; k++) {
          char* end = nullptr;
          radiance_ray[k < 3 ? k : k + 1] = std::strtof(argv[i + 1 + k], &end);
          six = end != argv[i + 1 + k] && *end == '\0';
        }
        if (!six) {
          std::fprintf(stderr, "--radiance needs six numbers: OX OY OZ DX DY DZ\n");
          return 2;
        }
        radiance = true;
        i += 5;
      } else if (!std::strcmp(argv[i], "--size")) {
        if (std::sscanf(argv[i + 1], "%dx%d", &size.x, &size.y) != 2) {  // WxH, or W H
          if (i + 2 >= argc || std::sscanf(argv[i + 1], "%d", &size.x) != 1 || std::sscanf(argv[i + 2], "%d", &size.y) != 1)
            return 2;
          i += 1;
        }
      } else {
        std::fprintf(stderr, "unknown option %s\n", argv[i]);
        return 2;
      }
    }
    if (no_image && !pick && !radiance) {
      std::fprintf(stderr, "no output image given\n");
      return 2;
    }
    if (samples > 0) settings.num_samples = (size_t)samples;
    const bool until = noise_target >= 0.f, adapt = adaptive >= 0.f;
    if (until && adapt) return 2;
    if ((until || adapt) && max_samples > 0) settings.num_samples = (size_t)max_samples;  // the bound, and the strata

    rt2::serialize::SceneLoader loader;
    auto scene_opt = loader.LoadScene(scene_path);
    if (!scene_opt.has_value()) {
      std::fprintf(stderr, "scene error: %s\n", loader.error.c_str());
      return 1;
    }
    rt2::Scene& scene = scene_opt.value();
    rt2::ivec2 dims{1600, 900};
    if (scene.dims.x != 0 && scene.dims.y != 0) dims = scene.dims;
    if (size.x > 0 && size.y > 0) dims = size;

    if (pick) {
      if (pick_at.x < 0 || pick_at.x >= dims.x || pick_at.y < 0 || pick_at.y >= dims.y) {
        std::fprintf(stderr, "--pick: pixel outside the %dx%d image\n", dims.x, dims.y);
        return 2;
      }
      // the feature pass's ray (rt2.h "Feature buffers and denoiser"), every operation rounded on its own
      float cp[21];
      rt2::Check(rt2_camera_params(scene.handle(), dims.x, dims.y, (int)settings.num_samples, cp));
      float v[3], ray[8], rec[16];
      for (int k = 0; k < 3; k++) {
        const float pc = (cp[k] + (float)pick_at.x * cp[3 + k]) + (float)pick_at.y * cp[6 + k];
        v[k] = pc - cp[9 + k];
        ray[k] = cp[9 + k];
      }
      const float inv = 1.0f / std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
      ray[3] = FLT_MAX;
      for (int k = 0; k < 3; k++) ray[4 + k] = v[k] * inv;
      ray[7] = 0.0f;
      rt2::RayTracer picker(scene, 0);
      picker.Intersect(ray, 1, rec);
      std::printf("{\"pick\": [%d, %d], \"size\": [%d, %d], \"record\": [", pick_at.x, pick_at.y, dims.x, dims.y);
      for (int k = 0; k < 16; k++) {  // nine digits round-trip a float; "-0.0", not "-0": a JSON reader keeps the sign
        char num[32];
        std::snprintf(num, sizeof num, "%.9g", (double)rec[k]);
        const bool integral = !std::strpbrk(num, ".e");
        std::printf("%s%s%s", k ? ", " : "", num, integral ? ".0" : "");
      }
      std::printf("]}\n");
      return 0;
    }

    if (radiance) {
      rt2_radiance_params prm = rt2::RayTracer::RadianceDefaults();
      prm.samples = samples > 0 ? (int)samples : 1;
      if (samples > 65535 || !rt2::RayTracer::RayValid(radiance_ray)) {
        std::fprintf(stderr, "--radiance needs a ray inside the query domain and --samples in [1, 65535]\n");
        return 2;
      }
      rt2::RayTracer probe(scene, 0);
      float sum[3];
      uint32_t cast = 0;
      probe.Radiance(radiance_ray, 1, sum, &cast, prm);
      std::printf("{\"samples\": %d, \"rays\": %u, \"radiance\": [", prm.samples, cast);
      for (int k = 0; k < 3; k++) {  // nine digits round-trip a float
        const float mean = sum[k] / (float)prm.samples;
        std::printf("%s%.9g", k ? ", " : "", (double)mean);
      }
      std::printf("]}\n");
      return 0;
    }

    if (ao_samples > 0) {
      if (no_image || gpus > 0) {
        std::fprintf(stderr, "--ao writes an image from one GPU\n");
        return 2;
      }
      rt2::RayTracer ao(scene, 0);
      scene.cam.SetSamplesPerPixel((int)settings.num_samples);
      ao.camera = &scene.cam;
      ao.OnResize(dims);
      std::vector<uint32_t> counts((size_t)dims.x * (size_t)dims.y);
      ao.Ambient(ao_samples, ao_radius, counts.data());
      std::vector<rt2::vec3> grey(counts.size());
      unsigned long long blocked = 0, hit_pixels = 0;
      for (size_t k = 0; k < counts.size(); k++) {
        const bool miss = counts[k] == 0xFFFFFFFFu;
        const float v = miss ? 1.0f : 1.0f - (float)counts[k] / (float)ao_samples;
        grey[k] = rt2::vec3{v, v, v};
        if (!miss) blocked += counts[k], hit_pixels++;
      }
      rt2::util::WriteImage(grey, dims.x, dims.y, out_path);
      std::printf("{\"ao_samples\": %d, \"width\": %d, \"height\": %d, \"hit_pixels\": %llu, \"blocked\": %llu, "
                  "\"kernel_ms\": %.3f}\n",
                  ao_samples, dims.x, dims.y, hit_pixels, blocked, ao.AmbientTime());
      return 0;
    }

    rt2::RayTracer tracer(scene, 0, gpus);
    tracer.max_depth = settings.max_depth;
    scene.cam.SetSamplesPerPixel((int)settings.num_samples);
    tracer.camera = &scene.cam;
    tracer.OnResize(dims);
    if (until || adapt || denoise) tracer.EnableMoments();
    if (adapt && gpus > 0) tracer.ImageEnableAdaptive();
    else if (adapt) tracer.EnableAdaptive();

    const auto t0 = std::chrono::steady_clock::now();
    if (until) {
      const rt2_noise nz = tracer.RenderUntil(scene, noise_target, (int)settings.num_samples);
      std::fprintf(stderr, "frames %zu rms %.9g\n", (size_t)tracer.FrameIdx(), (double)nz.rms);
    } else if (adapt) {
      const rt2_adaptive a = gpus > 0 ? tracer.ImageRenderAdaptive(scene, adaptive, (int)settings.num_samples, window)
                                      : tracer.RenderAdaptive(scene, adaptive, (int)settings.num_samples, window);
      std::fprintf(stderr, "frames %zu active %llu samples %llu\n", (size_t)tracer.FrameIdx(),
                   (unsigned long long)a.active, (unsigned long long)a.samples);
    } else {
      for (size_t i = 0; i < settings.num_samples; i++) tracer.Update(scene);
    }
    rt2_denoise_params dp = rt2::RayTracer::DenoiseDefaults();
    if (denoise_iterations > 0) dp.iterations = denoise_iterations;
    rt2_present_params pp = rt2::RayTracer::PresentDefaults();
    pp.temporal = 0;
    pp.denoise = 1;
    pp.dp = dp;
    // (each of the three runs the queued frames)
    const auto pixels = !denoise ? tracer.NonConvertedPixels() : gpus > 0 ? tracer.ImageResolve(&pp) : tracer.Denoise(&dp);
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    rt2::util::WriteImage(pixels, tracer.Dims().x, tracer.Dims().y, out_path);

    rt2_stats st{};
    rt2::Check(rt2_tracer_get_stats(tracer.handle(), &st));
    std::printf("{\"frames\": %zu, \"width\": %d, \"height\": %d, \"rays\": %llu, \"seconds\": %.6f, "
                "\"mray_s\": %.1f, \"launches\": %llu, \"gpus\": %d}\n",
                (size_t)tracer.FrameIdx(), dims.x, dims.y, (unsigned long long)st.rays, s, st.rays / s / 1e6,
                (unsigned long long)st.launches, tracer.NumGpus());
    if (until || adapt) return tracer.FrameIdx() >= 1 && tracer.FrameIdx() <= settings.num_samples ? 0 : 3;
    return tracer.FrameIdx() == settings.num_samples ? 0 : 3;
  } catch (const rt2::Error& e) {
    std::fprintf(stderr, "rt2 error %d: %s\n", e.code, e.what());
    return 1;
  }
}
