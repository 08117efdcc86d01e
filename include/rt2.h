/* rt2.h — C ABI of the MI355X (gfx950) replacement for the reference renderer's hot path.
 *
 * Drop-in boundary for tonadr1022/Raytrace2 `raytrace2::cpu::RayTracer` (src/cpu_raytrace/
 * RayTracer.hpp:15-42) and the host surface that stays around it: `serialize::SceneLoader`,
 * `LoadCamera`, `WriteCamera`, `LoadAppSettings` (src/Serialize.hpp:21-35) and
 * `util::WriteImage` (src/Util.hpp:11-12). Plain pointers and sizes only; no HIP or torch types in
 * the signatures (streams are passed as void*). Every function returns RT2_OK (0) or a negative
 * status and never throws; rt2_last_error() has the message (thread-local).
 *
 * Pixel layout: row-major, row 0 = bottom image row (RayTracer.cpp:97-102). With a row-band
 * partition (rt2_tracer_set_partition) a tracer owns the "local rows" y whose band b = y / band_h
 * has (b % world + b / world) % world == rank (one band per period of `world` bands, the phase
 * rotating by one each period), stored compactly in increasing y.
 */
#ifndef RT2_H_
#define RT2_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT2_API __attribute__((visibility("default")))

enum {
  RT2_OK = 0,
  RT2_ERR_INVALID = -1, /* bad argument or call order */
  RT2_ERR_IO = -2,      /* file missing / unreadable / unwritable */
  RT2_ERR_SCENE = -3,   /* scene schema or compile error */
  RT2_ERR_HIP = -4,     /* HIP runtime error (no device, out of memory, launch failure) */
};

typedef struct rt2_scene rt2_scene;
typedef struct rt2_tracer rt2_tracer;

RT2_API const char* rt2_last_error(void);
/* "rt2-mi355x <version> (gfx950) kernel <12 hex digits>": the last field identifies the kernel sources
 * (render.hip + rt2_layout.h) the library was built from */
RT2_API const char* rt2_version(void);

/* ---- SceneLoader::LoadScene (Serialize.cpp:199-360) + App.cpp:126 (top-level BVHNode) ----
 * Accepts the v2 schema and the legacy {"primitives":{"spheres":[...]}} schema (documented
 * adapter: each sphere is a top-level node; a missing camera means "cam1"). Camera names resolve
 * to <scene dir>/<name>.json. `seed` keys the Perlin-table random streams (the reference draws them
 * from its unseeded RNG at load, PerlinNoiseGen.cpp:41-50). */
RT2_API int rt2_scene_load(const char* path, uint64_t seed, rt2_scene** out);
/* The environment variable RT2_NO_LIST_ACCEL=1 at load keeps every list a linear child loop. */
RT2_API void rt2_scene_free(rt2_scene* scene);

typedef struct {
  int dims_x, dims_y; /* Scene::dims (camera width / aspect), 0 when absent */
  int n_materials, n_textures, n_primitives, n_top_nodes;
  float background[3];
  int legacy_schema;
  int bvh_nodes, quads, spheres, lists, xforms, media; /* flattened records */
  int max_stack, bvh_depth;
  uint64_t node_bytes;
  int acc_lists, acc_nodes; /* sphere lists given an exact acceleration tree, and its nodes */
  int linear_steps;         /* threaded-program length (0: the scene uses the stack traversal) */
  int origins_bounded;      /* 1: the threaded program's exact tests need camera rays starting within
                             * +-2^64 (rectangle quads, box boundaries, transforms about y); a launch
                             * refuses a camera beyond that (RT2_ERR_INVALID). 0: any camera renders */
  int box_steps;            /* MakeBox runs and MakeBox medium boundaries given the box-level test */
  int hit_table_bytes;      /* size of the scene's hit table (the shading records of its threaded program's
                             * quads, one flat record each, which the Cornell-box kernel stages in LDS); 0:
                             * none (RT2_HIT_TABLE=0 at load, nested transforms, no quad, or a table too
                             * large to stage without lowering the kernel's occupancy) */
  int flat_steps;           /* length of the scene's flat program (its threaded program without the BVH steps,
                             * walked with a per-lane certificate, DESIGN.md §4 "Flat walk of small BVHs"); 0:
                             * none (RT2_FLAT_BVH=0 at load, or the scene does not qualify: more than 8 BVH
                             * leaves, a sphere, a medium, a nested transform) */
} rt2_scene_info;
RT2_API int rt2_scene_get_info(const rt2_scene* scene, rt2_scene_info* out);
/* Material table, 8 floats per material: type, albedo.xyz, fuzz, refraction_index, tex_idx, 0.
 * type: 0 metal, 1 lambertian, 2 dielectric, 3 texture, 4 diffuse_light, 5 isotropic
 * (variant order of Fwd.hpp:13-14). Returns the material count. */
RT2_API int rt2_scene_materials(const rt2_scene* scene, float* out, int cap);
/* Texture table, 8 floats: type (0 solid, 1 checker, 2 noise), albedo.xyz, inv_scale|scale,
 * even, odd, noise_type. Returns the texture count. */
RT2_API int rt2_scene_textures(const rt2_scene* scene, float* out, int cap);
/* Perlin tables of noise texture `tex`: vec = point_count*3 floats, perm = 3*point_count ints
 * (perm_x, perm_y, perm_z). Returns point_count. */
RT2_API int rt2_scene_perlin(const rt2_scene* scene, int tex, float* vec, int* perm);

/* ---- Camera (Camera.hpp:10-137) ---- */
typedef struct {
  float center[3], look_at[3], view_up[3];
  float vfov, defocus_angle, focus_distance;
} rt2_camera_desc;
RT2_API int rt2_scene_get_camera(const rt2_scene* scene, rt2_camera_desc* out);
RT2_API int rt2_scene_set_camera(rt2_scene* scene, const rt2_camera_desc* cam);
/* Camera::Update for (w, h, spp): out[21] = pixel00(3) du(3) dv(3) center(3) defocus_u(3)
 * defocus_v(3) defocus_angle recip_sqrt_spp sqrt_spp */
RT2_API int rt2_camera_params(const rt2_scene* scene, int w, int h, int spp, float* out);
RT2_API int rt2_camera_load(const char* path, rt2_camera_desc* out);         /* LoadCamera */
RT2_API int rt2_camera_write(const rt2_camera_desc* cam, const char* path);  /* WriteCamera */

/* ---- LoadAppSettings (Serialize.cpp:56-65) ---- */
typedef struct {
  int render_once, save_after_render_once;
  int64_t num_samples, max_depth;
  int render_window;
} rt2_app_settings;
RT2_API int rt2_settings_load(const char* path, rt2_app_settings* out);

/* ---- RayTracer (RayTracer.hpp:15-42) on one GPU ----
 * create:   compiles the scene program and uploads it to `device` (the scene may be freed after).
 * on_resize:OnResize(dims) (RayTracer.cpp:87-104): sets camera dims, reallocates, Reset().
 * update:   Update(scene) (RayTracer.cpp:55-70): one frame, stratum (f % sq, f / sq % sq).
 * render:   n consecutive Update() calls, executed as ceil(n / launch_frames) kernel launches.
 * Update()/render() queue their frames; queued frames are launched together at the next readback,
 * query, synchronize or stats call, before a change of max_depth / spp / seed / stats mode, or once
 * `lazy_frames` (default 4096; 0 = launch at every call) are queued. Reset/OnResize drop queued
 * frames. Results are identical either way; FrameIdx() counts queued frames. Launched frames run on
 * the tracer's stream; readbacks synchronise it. */
RT2_API int rt2_tracer_create(const rt2_scene* scene, int device, rt2_tracer** out); /* n GPUs: see below */
RT2_API void rt2_tracer_destroy(rt2_tracer* tr);
RT2_API int rt2_tracer_set_stream(rt2_tracer* tr, void* hip_stream); /* NULL = own stream */
RT2_API int rt2_tracer_set_max_depth(rt2_tracer* tr, int max_depth); /* RayTracer::max_depth, <= 65535 */
RT2_API int rt2_tracer_set_samples_per_pixel(rt2_tracer* tr, int spp); /* App.cpp:129 */
RT2_API int rt2_tracer_set_seed(rt2_tracer* tr, uint64_t seed);
RT2_API int rt2_tracer_set_partition(rt2_tracer* tr, int band_h, int rank, int world);
RT2_API int rt2_tracer_set_launch_frames(rt2_tracer* tr, int frames_per_launch); /* 0 = all */
/* Work split: a launch's frames are cut into chunks and every (pixel, chunk) is one work item. A
 * chunk starting with R frames left holds about R * pixels / (k * resident GPU lanes) frames, k =
 * `items_per_lane` (default 4), at least 1 and at most 64 (RT2_CHUNK_MAX): long items early, short
 * ones at the end of the launch. 0 = one chunk (each pixel's frames in one item). Every frame's
 * sample goes to a per-frame buffer and is summed in frame order after the launch, so results do
 * not depend on the split. `bytes` bounds the device memory the samples take on each GPU in total
 * (default 24 GiB of the MI355X's 288 GB): consecutive launches alternate between two launch slots,
 * each with its own sample buffer of at most bytes / 2, so that a launch's tail overlaps the next
 * launch; a render needing more than bytes / 2 of samples runs as several launches (at least one
 * 8-frame octet each). rt2_stats.sample_buffer_bytes / device_bytes_peak report what is held. */
RT2_API int rt2_tracer_set_lazy_frames(rt2_tracer* tr, int max_queued);
RT2_API int rt2_tracer_flush(rt2_tracer* tr); /* launch the queued frames now (does not wait) */
RT2_API int rt2_tracer_set_work_split(rt2_tracer* tr, int items_per_lane);
RT2_API int rt2_tracer_set_sample_budget(rt2_tracer* tr, uint64_t bytes);
/* Most work items a GPU wave reserves with one atomic (default 64); batches shrink as the launch
 * drains. */
RT2_API int rt2_tracer_set_batch_max(rt2_tracer* tr, int items);
/* Launch shape of the last render: persistent workgroups, frames of its first chunk, kernel variant. */
RT2_API int rt2_tracer_last_launch(const rt2_tracer* tr, int* grid, int* chunk_frames, int* variant);
RT2_API int rt2_tracer_on_resize(rt2_tracer* tr, int width, int height);
RT2_API int rt2_tracer_reset(rt2_tracer* tr);
RT2_API int rt2_tracer_update(rt2_tracer* tr);
RT2_API int rt2_tracer_render(rt2_tracer* tr, int n_frames);
RT2_API int rt2_tracer_synchronize(rt2_tracer* tr);
RT2_API int64_t rt2_tracer_frame_idx(const rt2_tracer* tr); /* FrameIdx */
RT2_API int rt2_tracer_dims(const rt2_tracer* tr, int* width, int* height); /* Dims */
RT2_API int rt2_tracer_local_rows(const rt2_tracer* tr);
/* NonConvertedPixels (RayTracer.cpp:105-112): accum / frame_idx, float3 per local pixel */
RT2_API int rt2_tracer_non_converted_pixels(rt2_tracer* tr, float* out);
RT2_API int rt2_tracer_accumulation(rt2_tracer* tr, float* out); /* raw float3 sums */
RT2_API int rt2_tracer_pixels(rt2_tracer* tr, uint8_t* out_rgba); /* Pixels(): RGBA8 */
/* Progressive display (App.cpp:176-242 without the window): enqueue the Pixels() readback after the
 * frames already enqueued and return at once; the buffer is complete when rt2_tracer_query returns
 * 1 (all enqueued work done; 0 = still running) or after rt2_tracer_synchronize. Pinned host memory
 * from rt2_host_alloc makes the copy a DMA that does not stall the host. */
RT2_API int rt2_tracer_pixels_async(rt2_tracer* tr, uint8_t* out_rgba);
RT2_API int rt2_tracer_query(rt2_tracer* tr);
RT2_API int rt2_host_alloc(size_t bytes, void** out);
RT2_API void rt2_host_free(void* ptr);
/* Device-to-device copy of the local accumulation (float3 per local pixel) into `dst_device`,
 * ordered on `hip_stream` (NULL = tracer stream) — used for the multi-GPU gather. */
RT2_API int rt2_tracer_copy_accum_device(rt2_tracer* tr, void* dst_device, void* hip_stream);
/* ---- RayTracer::camera (RayTracer.hpp:31) ----
 * The reference borrows `Camera* camera` (= &scene.cam, App.cpp:130) and calls camera->Update() at
 * every Update() (RayTracer.cpp:56): a camera moved between Update() calls takes effect at the next
 * frame and does not reset the accumulation. set_camera gives the tracer the setter fields of
 * Camera.hpp:69-101 (center, look_at, view_up, vfov, defocus_angle, focus_distance; dims and
 * samples_per_pixel stay as on_resize / set_samples_per_pixel set them). When they change, frames
 * queued so far are launched first, with the camera they were queued under. Rendering refuses, with
 * RT2_ERR_INVALID, a camera whose rays would start beyond +-2^64 on an axis (center plus the defocus
 * disk): the kernel's exact axis-aligned rectangle test assumes ray origins within +-2^100. */
RT2_API int rt2_tracer_set_camera(rt2_tracer* tr, const rt2_camera_desc* cam);
RT2_API int rt2_tracer_get_camera(const rt2_tracer* tr, rt2_camera_desc* out);

/* ---- Multi-GPU; replaces the reference's data-parallel pixel loop
 * std::for_each(std::execution::par, ...) (RayTracer.cpp:69) ----
 * Pixels are independent and sample streams are keyed by (seed, global pixel, frame), so the image
 * is split into interleaved row bands (band b -> GPU b % n) and rendered with no communication. The
 * one exchange is an RCCL gather (ncclGather over xGMI) of every GPU's band stack to the root GPU,
 * where a kernel de-interleaves it into the full image. The result is bit-identical to one GPU.
 *
 * (1) One process driving n GPUs: rt2_tracer_create_multi (devices NULL = 0..n-1; band_h 0 = 2),
 *     one RCCL communicator per device (ncclCommInitAll). Every rt2_tracer_* function works on it as
 *     on a one-GPU tracer; readbacks (accumulation, non_converted_pixels, pixels, pixels_async,
 *     ray_counts, copy_accum_device) return the FULL image (local_rows = height), gathering first.
 *     set_stream, set_partition and join are refused. A device listed more than once runs several
 *     partitions on one GPU with device-local copies in place of RCCL (a test configuration).
 * (2) One process per GPU (torchrun / MPI style): each process creates a one-GPU tracer; rank 0 makes
 *     an id with rt2_comm_unique_id, the caller broadcasts it, and every rank calls rt2_tracer_join
 *     (= set_partition(band_h, rank, world) + ncclCommInitRank). Readbacks stay local (the rank's
 *     bands); rt2_tracer_gather is the collective that assembles the full image on rank 0, read
 *     there with rt2_tracer_image_*.
 * rt2_tracer_gather works in both modes. It is enqueued on the tracers' streams and does not wait. */
#define RT2_UNIQUE_ID_BYTES 128
RT2_API int rt2_tracer_create_multi(const rt2_scene* scene, int n_gpus, const int* devices, int band_h,
                                    rt2_tracer** out);
RT2_API int rt2_tracer_n_gpus(const rt2_tracer* tr); /* devices of a multi tracer, else 1 */
/* rt2_tracer_create_multi's argument checks and partition, on the host only (no GPU, no RCCL): part
 * i = rank i on devices[i] renders local_rows rows of the image in bands of band_h rows (0 = 2), and
 * every part sends rows_max rows in the gather. loopback = 1 when every device is one GPU (the tests'
 * configuration: device-local copies instead of RCCL). out may be NULL (checks only). */
typedef struct {
  int device, rank, world, band_h;
  int local_rows; /* image rows this part renders */
  int rows_max;   /* rows of the largest part's band stack: what every part sends */
} rt2_part_plan;
RT2_API int rt2_multi_plan(int n_gpus, const int* devices, int band_h, int width, int height, rt2_part_plan* out,
                           int* loopback);
RT2_API int rt2_comm_unique_id(uint8_t* out, size_t cap); /* cap >= RT2_UNIQUE_ID_BYTES */
RT2_API int rt2_tracer_join(rt2_tracer* tr, const uint8_t* unique_id, int world, int rank, int band_h);
RT2_API int rt2_tracer_gather(rt2_tracer* tr);
/* Root (rank 0 / a multi tracer) after a gather: the full image, rows bottom-up, H x W. */
RT2_API int rt2_tracer_image_accumulation(rt2_tracer* tr, float* out);        /* raw float3 sums */
RT2_API int rt2_tracer_image_non_converted_pixels(rt2_tracer* tr, float* out); /* accum / frame_idx */
/* NonConvertedPixels of the gathered image enqueued on the root's stream into pinned host memory
 * (rt2_host_alloc); complete when rt2_tracer_query returns 1 or after rt2_tracer_synchronize. */
RT2_API int rt2_tracer_image_non_converted_pixels_async(rt2_tracer* tr, float* out);
RT2_API int rt2_tracer_image_pixels(rt2_tracer* tr, uint8_t* out_rgba);       /* Pixels(): RGBA8 */
/* The gather's layout, for callers that move the band stacks themselves (e.g. over another
 * collective library): every rank sends rt2_band_rows_max(height, band_h, world) rows of its band
 * stack (padding rows zero); rt2_deinterleave_host turns the rank-major stacks
 * [world][max_rows][width][channels] (what ncclGather delivers on the root) into the image
 * [height][width][channels] on the host, with the same index map as the root's de-interleave
 * kernel (rt2_layout.h BandSource). No GPU needed. */
RT2_API int rt2_band_rows_max(int height, int band_h, int world);
RT2_API int rt2_deinterleave_host(const float* stacks, float* image, int width, int height, int band_h, int world,
                                  int max_rows, int channels);
/* The RCCL and HIP runtime this process runs (the first library of each name loaded wins: under
 * PyTorch that is torch's bundled copy, in a plain C++ process the one librt2.so was linked with):
 * writes "rccl <version> <path>; hip <path>" into out. */
RT2_API int rt2_runtime_info(char* out, size_t cap);

RT2_API int rt2_tracer_enable_ray_counts(rt2_tracer* tr, int on);
RT2_API int rt2_tracer_ray_counts(rt2_tracer* tr, uint32_t* out); /* rays per local pixel */
RT2_API int rt2_tracer_enable_stats(rt2_tracer* tr, int on);      /* per-record test counters */

typedef struct {
  uint64_t rays;      /* closest-hit queries issued by RayColor (depth > 0) */
  uint64_t paths;     /* camera samples finished */
  uint64_t bvh_tests, quad_tests, sphere_tests, xform_visits, medium_tests, list_visits;
  uint64_t overflow;  /* lanes that hit the traversal-stack bound (must be 0) */
  uint64_t launches;
  /* render-kernel GPU time: the time in which at least one render launch ran, each launch timed by
   * its own clock from its first wave's start to its last wave's end (queue time excluded;
   * consecutive launches overlap in the previous launch's tail, counted once) */
  double kernel_ms;
  uint64_t stamps[4]; /* diagnostic builds only: s_memtime sums (fetch, trace, shade, finish) */
  uint64_t diag[8];   /* diagnostic builds only: per-wave traversal step counts */
  /* multi-GPU (root): gathers done, and the sum of their root-stream durations (HIP events from the
   * root's last render kernel to the de-interleaved image; waiting for the slowest GPU included).
   * For a multi-GPU tracer the counters above are sums over its GPUs, except launches (per GPU)
   * and kernel_ms (the largest per-GPU sum). */
  uint64_t gathers;
  double gather_ms;
  /* host time spent enqueueing renders (a multi-GPU tracer: sum over its GPUs); image readbacks to
   * the host (rt2_tracer_image_*) on the root and their device-to-host copy time */
  double enqueue_ms;
  uint64_t readbacks;
  double readback_ms;
  /* times the library blocked the host on the GPU (stream / event synchronizations); the launch path
   * (Render, flush, gather, the async readbacks) adds none */
  uint64_t host_waits;
  /* the sum of the render launches' first-wave-to-last-wave times (>= kernel_ms: overlaps counted
   * once per launch) */
  double launch_ms_sum;
  /* device memory: both launch slots' per-frame sample buffers now (<= the sample budget), and the
   * high-water mark of everything this tracer holds on its GPU (scene program, frame buffers, sample
   * buffers, chunk tables, a root's gathered image). A multi-GPU tracer: the largest GPU's. */
  uint64_t sample_buffer_bytes;
  uint64_t device_bytes_peak;
  /* stats mode, the box-level test of MakeBox runs (sphere scenes): lanes tested and certified (the others
   * fall back to the six-face run), wave visits of a flagged run and those in which the wave ran the six
   * faces for its uncertified lanes */
  uint64_t box_tests, box_certified, box_wave_visits, box_wave_runs;
  /* bytes of the scene's hit table the last render launch staged in LDS; 0: that launch read the records
   * from global memory (no table, a kernel that takes none, such as the counting kernels, or a table that
   * would have lowered the kernel's occupancy) */
  uint64_t hit_table_bytes;
  /* the flat walk (launches over a scene's flat program; counted in every such launch, 0 otherwise): lanes
   * whose hit the certificate left open, and wave-bounces that traced the BVH program again for them.
   * flat_fallback_hits: the hits those wave-bounces ended with, over all their lanes. RT2_FLAT_BVH=2 at scene
   * load certifies no hit: every wave-bounce with a hit falls back, and both flat_uncertified and
   * flat_fallback_hits are the number of hits */
  uint64_t flat_uncertified, flat_wave_fallbacks, flat_fallback_hits;
} rt2_stats;
RT2_API int rt2_tracer_get_stats(rt2_tracer* tr, rt2_stats* out);
/* The stats of GPU `part` of a multi-GPU tracer (part 0 of a one-GPU tracer is itself). */
RT2_API int rt2_tracer_part_stats(rt2_tracer* tr, int part, rt2_stats* out);
RT2_API int rt2_tracer_reset_stats(rt2_tracer* tr);

/* ---- Noise estimate and render-until-converged (DESIGN.md "Noise estimate") ----
 * Opt-in "moments": with them on, the pass that sums a launch's samples in frame order also sums
 * their squares (float32, q = q + s * s per channel, each operation rounded on its own), so both sums
 * are defined in frame order and do not depend on how frames were split into launches. With moments
 * off nothing changes. From n = FrameIdx() >= 2 frames and a pixel's sums a_c (accumulation) and q_c
 * (moment2), in double with every operation rounded on its own:
 *   mean_c = a_c / n;  ss_c = q_c - a_c * mean_c, 0 unless > 0
 *   sem_c  = (float) sqrt(ss_c / ((double)n * (n - 1)))          standard error of the mean
 *   err    = sqrt((sem_r^2 + sem_g^2 + sem_b^2) / 3) / max(1, (mean_r + mean_g + mean_b) / 3)
 * A pixel with a non-finite a_c or q_c has sem = err = +inf; it counts as `nonfinite`, never as
 * `below`, and is left out of sum_sq and max_err. The scalars are reduced without atomics in a fixed
 * order: the same image gives the same bytes every time.
 * enable_moments: like enable_ray_counts it synchronises, reallocates and resets the frame index and
 *   the accumulation. Reset / OnResize zero the sums of squares too.
 * moments / standard_error / noise: readbacks (they launch queued frames and synchronise);
 *   RT2_ERR_INVALID with moments off, and for standard_error / noise with fewer than 2 frames.
 * render_until: renders in steps of `check_every` frames (0: one stratum sweep, sqrt_spp^2 frames; the
 *   last step shortened to land on max_frames) while FrameIdx() < max_frames; after each step with
 *   FrameIdx() >= max(min_frames, 2) it takes the noise (threshold = target_rms) and stops when
 *   rms <= target_rms and nonfinite == 0. FrameIdx() counts from the last reset, so an accumulation
 *   already begun is continued. `out` receives the last estimate (frames = 0: none could be taken).
 *   The image afterwards is, bit for bit, that of Render(FrameIdx()).
 * Multi-GPU: a create_multi tracer forwards enable_moments; moments / standard_error return the full
 *   image (each GPU's rows placed on the host, as ray_counts); noise adds the GPUs' pixels, below,
 *   nonfinite and sum_sq, takes the largest max_err and recomputes rms. A joined tracer (one process
 *   per GPU) reports its own bands: the additive fields are what the caller all-reduces. */
typedef struct {
  int64_t frames;     /* n the estimate rests on */
  uint64_t pixels;    /* local pixels (a multi-GPU tracer: the whole image) */
  uint64_t below;     /* pixels with err <= threshold */
  uint64_t nonfinite;
  double sum_sq;      /* sum of err^2 over the finite pixels */
  float max_err;      /* largest finite err */
  float rms;          /* sqrt(sum_sq / (pixels - nonfinite)), 0 when that is 0 */
} rt2_noise;
RT2_API int rt2_tracer_enable_moments(rt2_tracer* tr, int on);
RT2_API int rt2_tracer_moments(rt2_tracer* tr, float* out);        /* raw float3 sums of squares, local pixels */
RT2_API int rt2_tracer_standard_error(rt2_tracer* tr, float* out); /* float3 sem per local pixel */
RT2_API int rt2_tracer_noise(rt2_tracer* tr, float threshold, rt2_noise* out);
RT2_API int rt2_tracer_render_until(rt2_tracer* tr, float target_rms, int min_frames, int max_frames, int check_every,
                                    rt2_noise* out);

/* ---- Adaptive sampling (DESIGN.md "Adaptive sampling") ----
 * Opt-in, needs moments on; with it off nothing changes. Pixels whose noise estimate has met a threshold
 * retire and later launches trace only the rest. Sample streams are keyed by (seed, global pixel, frame)
 * and summed in frame order, so a pixel that stops after n frames holds exactly the sums of Render(n).
 * State per local pixel: a sample count n_p (uint32) and an active flag.
 * enable_adaptive: like enable_moments it synchronises, reallocates and resets the frame index and the
 *   sums; afterwards every pixel is active and n_p = 0. Reset / OnResize / set_partition reactivate every
 *   pixel and zero the counts.
 * Rendering: Update() / Render(n) advance FrameIdx() by n as always. The frames [F, F + n) are traced
 *   only for the active pixels: a += s, q += s * s, n_p += n. An active pixel always has n_p ==
 *   FrameIdx(); a retired pixel keeps the count and the sums it had when it retired. While every pixel
 *   is active a launch is the launch it always was; with none active nothing is launched and the frame
 *   index still advances.
 * adaptive_check(threshold, window): needs FrameIdx() >= 2; launches queued frames first. For every local
 *   pixel err_p = the noise estimate above from (a_p, q_p, n_p), and over_p = !(finite_p && err_p <=
 *   (double)threshold): a non-finite pixel is always over. An active pixel at column x stays active iff
 *   some pixel of the same row in the columns [x - window, x + window] within [0, width) is over;
 *   otherwise it retires and stays retired until the next reset. 0 <= window <= 64. The window runs
 *   along the row only: partitions hold whole rows, so the decision needs no other GPU's pixels and is the
 *   same under any set_partition. (Why a window: a pixel that has seen only black samples so far has
 *   err exactly 0; window 0 would freeze it black, window 1 keeps it going while a neighbour is noisy.)
 * render_adaptive: renders in steps of `check_every` frames (0: one stratum sweep; the last step
 *   shortened to land on max_frames) while FrameIdx() < max_frames; after each step with FrameIdx() >=
 *   max(min_frames, 2), the last one included, it runs a check and stops when no pixel is active. `out`
 *   receives the last check (frames = 0: no step ended in one).
 * Readbacks with adaptive on: sample_counts returns n_p per local pixel; non_converted_pixels and the
 *   RGBA pixels divide by (float)n_p instead of the frame index; standard_error and noise use each
 *   pixel's own n_p (rt2_noise.frames stays FrameIdx()); accumulation, moments and ray_counts are the raw
 *   sums as always (a pixel's ray count is that of its first n_p frames).
 * Contract: for every pixel (a_p, q_p) equal, bit for bit, what a tracer without adaptive sampling holds
 *   after Render(n_p).
 * Caveat: stopping on a pixel's own variance estimate is biased — an unlucky pixel whose first samples
 *   happen to agree looks converged and freezes. `window` and `min_frames` are the guards.
 * RT2_ERR_INVALID: enable_adaptive with moments off, or on a create_multi or joined tracer (their gathered
 *   image divides by one common frame index; set_partition tracers work, and "Adaptive sampling of the gathered
 *   image" below is the family for those tracers); enable_moments(0) and join while
 *   adaptive is on; sample_counts / adaptive_check / render_adaptive with adaptive off; a check with
 *   fewer than 2 frames; a window outside [0, 64] or a threshold that is negative or NaN; enable_adaptive
 *   on a tracer that renders without the threaded traversal (the list kernels exist for that mode only).
 * Every field of rt2_adaptive but `frames` is additive over partitions. */
typedef struct {
  int64_t frames;     /* FrameIdx() at the check */
  uint64_t pixels;    /* local pixels */
  uint64_t active;    /* pixels still active after this check */
  uint64_t retired;   /* pixels this check retired */
  uint64_t samples;   /* sum of n_p */
  uint64_t nonfinite; /* pixels with a non-finite sum (never retired) */
} rt2_adaptive;
RT2_API int rt2_tracer_enable_adaptive(rt2_tracer* tr, int on);
RT2_API int rt2_tracer_sample_counts(rt2_tracer* tr, uint32_t* out); /* n_p per local pixel */
RT2_API int rt2_tracer_adaptive_check(rt2_tracer* tr, float threshold, int window, rt2_adaptive* out);
RT2_API int rt2_tracer_render_adaptive(rt2_tracer* tr, float threshold, int window, int min_frames, int max_frames,
                                       int check_every, rt2_adaptive* out);

/* ---- Feature buffers and denoiser ----
 * Opt-in: a tracer that never calls these allocates nothing new and launches what it launched before.
 * features: the scene's Hit (HitRecord) for the ray through each local pixel's centre, 16 floats per local
 *   pixel in the row order of `accumulation`. With the words of rt2_camera_params, for the pixel at image
 *   (x, y): pc = (pixel00 + (float)x * du) + (float)y * dv, origin = center (no defocus offset, whatever the
 *   camera's defocus_angle), d = normalize(pc - center), time 0, interval (0.001, FLT_MAX), every operation
 *   rounded on its own. Slots: 0 hit (0 / 1); 1 t; 2-4 point; 5-7 normal (facing against the ray); 8
 *   front_face; 9 material index; 10-12 albedo; 13 dist = sqrt(dot(point - center, point - center)); 14-15 0.
 *   Albedo: the material table's albedo (metal, lambertian), (1, 1, 1) (dielectric), Texture::Value at the
 *   hit (texture, diffuse_light, isotropic). A miss: slot 0 = 0, albedo = the background, every other slot 0.
 *   t is model-space under a transformed child (the reference's quirk); the filter uses dist and the point.
 *   A ConstantMedium on the way draws from the path stream (tracer seed, pixel 0xFFFFFFF0, frame 0) from its
 *   start, the same for every pixel: a medium's boundary in the feature image is the reference's
 *   probabilistic hit, not a geometric surface. The buffer is cached on the device per (camera, size,
 *   partition, seed); it works under set_partition on the local rows.
 * denoise: an edge-avoiding a-trous wavelet filter (raytrace2_amd/csrc/denoise.h defines every operation)
 *   over the tracer's mean image, guided by the features and weighted by the variance of the mean. Inputs,
 *   exactly what the readbacks return: c = non_converted_pixels, v = ((sem_r^2 + sem_g^2) + sem_b^2) / 3 in
 *   float32 from standard_error (adaptive sampling: both rest on each pixel's own n_p). Needs moments on,
 *   FrameIdx() >= 2 and an unpartitioned one-GPU tracer (world 1, not joined). It launches queued frames and
 *   synchronises; accumulation, moments, counts and FrameIdx() are unchanged. out_color: float3 per pixel;
 *   out_variance: float per pixel, the filtered variance of the mean, or NULL.
 * denoise_buffers: the same kernels over caller (host) buffers of any image: color float3, variance float,
 *   features 16 floats per pixel, on `device`.
 * A pixel whose colour or variance is not finite passes through unchanged and contributes to no other pixel.
 * RT2_ERR_INVALID: features / denoise on a create_multi or joined tracer (gathering features is a
 *   follow-up); denoise with moments off, fewer than 2 frames or a partition (world > 1); iterations outside
 *   [1, 8], normal_power_log2 outside [0, 8], a sigma or eps_l that is not finite and > 0; a NULL out_color;
 *   features on a scene only the threaded traversal can render (a stack deeper than the kernel's).
 * The environment variable RT2_DENOISE_LDS=0 / 1 (read at every call) takes the small steps' LDS tiles off /
 * on (same results; tools/denoise_cost.py measures both). */
typedef struct {
  int iterations;         /* 1..8, default 5: pass i has step 1 << i */
  int normal_power_log2;  /* 0..8, default 7: max(0, dot(n_p, n_q)) squared this many times */
  float sigma_l;          /* default 1: luminance tolerance in standard errors of the mean */
  float sigma_p;          /* default 0.01: plane-distance tolerance as a fraction of the hit's distance */
  float sigma_a;          /* default 0.1: albedo tolerance */
  float eps_l;            /* default 1e-3: luminance tolerance floor */
} rt2_denoise_params;     /* NULL = defaults */
RT2_API void rt2_denoise_defaults(rt2_denoise_params* out);
RT2_API int rt2_tracer_features(rt2_tracer* tr, float* out); /* 16 floats per local pixel */
RT2_API int rt2_tracer_denoise(rt2_tracer* tr, const rt2_denoise_params* p, float* out_color,
                               float* out_variance /* may be NULL */);
RT2_API int rt2_denoise_buffers(int device, int width, int height, const float* color, const float* variance,
                                const float* features, const rt2_denoise_params* p, float* out_color,
                                float* out_variance /* may be NULL */);
/* GPU time (HIP events on the tracer's stream) of the tracer's last feature pass and of the kernels of its
 * last denoise call, in ms; -1: none yet. */
RT2_API int rt2_tracer_denoise_times(rt2_tracer* tr, double* features_ms, double* denoise_ms);

/* ---- Temporal reuse ----
 * Opt-in: a tracer that never calls these allocates nothing new and launches what it launched before.
 * The image history reprojected across a camera move: each pixel's first-hit point (feature slots 2-4) is
 * projected into the camera the history was taken under, the history is read there with bilinear weights from
 * the taps whose old first hit is the same surface (material index, normal, plane distance, albedo), and
 * blended with the current estimate in proportion to the two lengths (frames). raytrace2_amd/csrc/temporal.h
 * defines every operation; float32, bit for bit the same on the GPU, the host and in numpy.
 * temporal_buffers: the kernels over caller (host) buffers of any image on `device`: the current color float3,
 *   variance float (of the mean), length float (frames, >= 0) and features (16 floats) per pixel; the same four
 *   of the history (length 0: none) with the 21 words of rt2_camera_params it was taken under; the material
 *   table of rt2_scene_materials (8 floats each) or NULL (every material diffuse). out_variance and out_length
 *   may be NULL.
 * temporal_resolve: a readback of the tracer's estimate blended with its history. Inputs as rt2_tracer_denoise
 *   takes them (c = non_converted_pixels, v from standard_error), n = (float)FrameIdx() or each pixel's own n_p
 *   under adaptive sampling, the tracer's features. With no history held the current estimate comes back
 *   with length n (0 at a pixel that is not finite). denoise != 0: rt2_tracer_denoise's filter (dp, NULL =
 *   defaults) then runs over the blended colour and variance with the current features, and the filtered
 *   colour and variance are returned; out_length is the blend's. Needs what rt2_tracer_denoise needs: moments
 *   on, FrameIdx() >= 2, an unpartitioned one-GPU tracer. It launches queued frames and synchronises; the
 *   history, accumulation, moments, counts and FrameIdx() are unchanged: a second call returns the same bytes.
 * temporal_push: the same blend, never filtered, becomes the history, with the current features and camera
 *   words; it replaces the previous history. Call it right before set_camera + reset.
 * The history survives reset and set_camera; on_resize, enable_moments, enable_adaptive, set_partition
 *   (which reallocate) and temporal_clear drop it.
 * temporal_time: GPU time (HIP events) of the last resolve's temporal kernels (inputs and blend; not the
 *   feature pass, not the filter), in ms; -1: none yet.
 * RT2_ERR_INVALID: resolve / push / clear on a create_multi, joined or partitioned tracer; resolve / push with
 *   moments off or fewer than 2 frames; max_history, sigma_p or sigma_a not finite and > 0,
 *   max_history_specular not finite and >= 0, min_normal_dot not finite; a NULL out_color; temporal_buffers
 *   with width or height <= 0, width * height >= 2^26, n_materials < 0 or a NULL input. */
typedef struct {
  float max_history;          /* default 1024: the longest history a pixel carries, in frames */
  float max_history_specular; /* default 0: the same where the current first hit is a metal or a dielectric */
  float min_normal_dot;       /* default 0.9: least dot of the current and the old normal */
  float sigma_p;              /* default 0.01: plane-distance tolerance as a fraction of the hit's distance */
  float sigma_a;              /* default 0.1: albedo tolerance */
} rt2_temporal_params;        /* NULL = defaults */
RT2_API void rt2_temporal_defaults(rt2_temporal_params* out);
RT2_API int rt2_temporal_buffers(int device, int width, int height, const float* color, const float* variance,
                                 const float* length, const float* features, const float* hist_color,
                                 const float* hist_variance, const float* hist_length, const float* hist_features,
                                 const float* hist_camera /* 21 words */, const float* materials /* may be NULL */,
                                 int n_materials, const rt2_temporal_params* p, float* out_color, float* out_variance,
                                 float* out_length);
RT2_API int rt2_tracer_temporal_resolve(rt2_tracer* tr, const rt2_temporal_params* p, int denoise,
                                        const rt2_denoise_params* dp, float* out_color,
                                        float* out_variance /* may be NULL */, float* out_length /* may be NULL */);
RT2_API int rt2_tracer_temporal_push(rt2_tracer* tr, const rt2_temporal_params* p);
RT2_API int rt2_tracer_temporal_clear(rt2_tracer* tr);
RT2_API int rt2_tracer_temporal_time(rt2_tracer* tr, double* resolve_ms);

/* ---- Presenting reconstructed frames ----
 * Opt-in: a tracer that never calls these allocates nothing new and launches what it launched before.
 * The display path of the reconstruction: what rt2_tracer_pixels_async is to the raw accumulation. Every call
 * but `present` and `present_buffers` only enqueues on the tracer's stream and returns at once; none of them
 * adds to rt2_stats.host_waits.
 * present_async: enqueues, in this order, the queued frames (as rt2_tracer_flush), the feature pass if its cache
 *   is stale, the inputs of rt2_tracer_denoise (c = non_converted_pixels, v from standard_error; each pixel's
 *   own n_p under adaptive sampling), if `temporal` rt2_tracer_temporal_resolve's blend with the held history
 *   (none held: the current estimate), if `denoise` rt2_tracer_denoise's filter, the tone map
 *   (raytrace2_amd/csrc/present.h: per channel v = c > 0 ? c : 0, v = v < 1 ? v : 1, byte = floor((double)v *
 *   255.999), alpha 255: Pixels()'s arithmetic, defined for every input: NaN -> 0, +inf -> 255, -inf -> 0) and
 *   a copy of 4 * width * height bytes into out_rgba. The buffer is complete when rt2_tracer_query returns 1 or
 *   after rt2_tracer_synchronize; pinned memory from rt2_host_alloc makes the copy a DMA. With both stages off
 *   the bytes are those of rt2_tracer_pixels. Needs what temporal_resolve needs, decided on the host without a
 *   wait (FrameIdx() counts queued frames): moments on, FrameIdx() >= 2, an unpartitioned one-GPU tracer. The
 *   accumulation, moments, counts, history and FrameIdx() are unchanged. Later calls reuse the tracer's scratch;
 *   stream order makes several presents in flight into different buffers safe.
 * present: present_async, then rt2_tracer_synchronize.
 * move_camera: temporal_push, set_camera and reset in one call, without a wait. With moments on and
 *   FrameIdx() >= 2 on an unpartitioned tracer the blend (tp, NULL = defaults) becomes the history, taken under
 *   the camera the frames were rendered with; otherwise (also on a set_partition tracer) it is set_camera +
 *   reset, and a history already held is kept. The reset's zeroing runs on the tracer's stream behind the push.
 * present_time: GPU time (HIP events) of the last present's kernels (inputs, blend, filter, tone map; not the
 *   render, the feature pass or the copy), in ms; -1 while that present has not finished, or when there was
 *   none. It polls the event and never waits.
 * present_buffers: the tone map alone over a caller (host) float3 image on `device`; it blocks, like
 *   rt2_denoise_buffers.
 * RT2_ERR_INVALID: any of the four tracer calls on a create_multi or joined tracer, and all but move_camera on a
 *   partitioned one; present / present_async with moments off or fewer than 2 frames, or with invalid temporal
 *   or denoise parameters (checked only for the stages switched on); move_camera with invalid temporal
 *   parameters; a NULL tracer, output or camera; present_buffers with width or height <= 0, width * height >=
 *   2^26 or a NULL argument. A refused call changes nothing. */
typedef struct {
  int temporal;            /* default 1: blend with the history (rt2_tracer_temporal_resolve's blend) */
  int denoise;             /* default 1: then rt2_tracer_denoise's filter */
  rt2_temporal_params tp;  /* defaults of rt2_temporal_defaults */
  rt2_denoise_params dp;   /* defaults of rt2_denoise_defaults */
} rt2_present_params;      /* NULL = defaults */
RT2_API void rt2_present_defaults(rt2_present_params* out);
RT2_API int rt2_tracer_present_async(rt2_tracer* tr, const rt2_present_params* p, uint8_t* out_rgba);
RT2_API int rt2_tracer_present(rt2_tracer* tr, const rt2_present_params* p, uint8_t* out_rgba);
RT2_API int rt2_tracer_move_camera(rt2_tracer* tr, const rt2_camera_desc* cam, const rt2_temporal_params* tp);
RT2_API int rt2_tracer_present_time(rt2_tracer* tr, double* ms);
RT2_API int rt2_present_buffers(int device, int width, int height, const float* color, uint8_t* out_rgba);

/* ---- Reconstructing the gathered image ----
 * Opt-in: a tracer that never calls these allocates nothing new and launches what it launched before
 * (rt2_tracer_gather included). The three sections above, for the image a create_multi or joined tracer gathers
 * on rank 0: the rt2_tracer_image_* family means "of the gathered image, on its root". They also work on a plain
 * one-GPU tracer (world 1), whose gather is a device-local copy. The calls above keep their refusals on these
 * tracers. Every result is bit for bit what a one-GPU tracer returns from the call named beside it at the same
 * seed, size, camera and frame count.
 * gather_estimate: rt2_tracer_gather with the sums of squares: every rank's stack of moments travels with its
 *   accumulation (the same RCCL group; on one GPU, copies on the root's stream, and every part's stream waits for
 *   an event recorded after both copies), and one kernel on the root writes what gather's kernel writes
 *   (image_accumulation, image_non_converted_pixels and image_pixels read the same bytes) and the variance of the
 *   mean. Collective on joined tracers: every rank calls it. It enqueues and does not wait. Needs moments on on
 *   every rank, FrameIdx() >= 2 and adaptive sampling off (or switched on by rt2_tracer_image_enable_adaptive:
 *   "Adaptive sampling of the gathered image" below).
 * image_variance: blocking readback of v = ((sem_r^2 + sem_g^2) + sem_b^2) / 3 in float32, float per image pixel:
 *   what rt2_tracer_denoise takes from standard_error.
 * image_features: rt2_tracer_features of the whole image, 16 floats per image pixel, traced on the root alone (the
 *   records are not gathered: DESIGN.md §6h) and cached there per (camera, seed, size). Blocks. Needs no gather
 *   and no moments.
 * image_resolve: rt2_tracer_temporal_resolve and rt2_tracer_denoise in one, over c = image_non_converted_pixels and
 *   v = image_variance: if p->temporal the blend with the root's whole-image history (none held: the current
 *   estimate, length (float)FrameIdx()), if p->denoise the filter over the result. p NULL = the defaults (both on).
 *   Blocks. out_variance, out_length may be NULL; out_length is the blend's length and is left untouched with
 *   temporal = 0. The history and the estimate are unchanged.
 * image_present_async / image_present / image_present_time: rt2_tracer_present_async, present and present_time
 *   over the same buffers: inputs, blend, filter, tone map and the copy of 4 * width * height bytes, enqueued on
 *   the root's stream; complete when rt2_tracer_query returns 1 or after rt2_tracer_synchronize. The async form
 *   only enqueues, refuses before its first enqueue and adds nothing to rt2_stats.host_waits. With both stages off
 *   the bytes are those of image_pixels.
 * image_move_camera: rt2_tracer_move_camera: with moments on and FrameIdx() >= 2 the blend (tp, NULL = defaults)
 *   of the current gathered estimate becomes the root's history under the camera it was rendered with; then
 *   set_camera and reset on every part. Otherwise set_camera + reset, and a history held is kept. The host does
 *   not wait. Collective on joined tracers: every rank calls it, a rank whose last gather_estimate is not of the
 *   current FrameIdx() takes part in one, and ranks other than 0 then set the camera and reset.
 * The history survives reset and set_camera; on_resize, enable_moments and set_partition drop it.
 * When the estimate must be current: on a create_multi or plain tracer image_resolve, image_present* and
 *   image_move_camera run gather_estimate themselves when the estimate held is not that of the current FrameIdx()
 *   (queued frames included). On a joined tracer image_resolve and image_present* are refused unless a
 *   gather_estimate of the current FrameIdx() has been enqueued (the other ranks are not in this process).
 * deinterleave_estimate_host: the CPU statement of gather_estimate's kernel, beside rt2_deinterleave_host: the
 *   rank-major stacks [world][rt2_band_rows_max][width][3] of the sums and of the sums of squares -> the image-order
 *   sums `image`, the means `image_nc` = sum / (float)frames (float3 each) and `variance` (float). No GPU needed.
 * RT2_ERR_INVALID: a NULL tracer, camera or output (out_variance, out_length excepted); a readback, resolve,
 *   present or present_time on a rank other than 0; gather_estimate (and the calls that run it) with moments off,
 *   fewer than 2 frames, adaptive sampling switched on by rt2_tracer_enable_adaptive, on a set_partition tracer (world > 1) that is not joined, or with
 *   ranks that disagree on dims or frame index; image_variance before any gather_estimate; image_resolve /
 *   image_present* on a joined tracer without a gather_estimate of the current FrameIdx(); invalid temporal or
 *   denoise parameters, checked only for the stages switched on (image_move_camera: its temporal parameters);
 *   image_features, resolve, present and a pushing move_camera on a scene only the threaded traversal can render;
 *   image_move_camera with adaptive sampling switched on by rt2_tracer_enable_adaptive or on an unjoined partition; deinterleave_estimate_host with a
 *   NULL argument, a negative size, world < 1 or frames outside [2, 2^31). A refused call changes nothing. */
RT2_API int rt2_tracer_gather_estimate(rt2_tracer* tr);
RT2_API int rt2_tracer_image_variance(rt2_tracer* tr, float* out);  /* float per image pixel */
RT2_API int rt2_tracer_image_features(rt2_tracer* tr, float* out);  /* 16 floats per image pixel */
RT2_API int rt2_tracer_image_resolve(rt2_tracer* tr, const rt2_present_params* p, float* out_color,
                                     float* out_variance /* may be NULL */, float* out_length /* may be NULL */);
RT2_API int rt2_tracer_image_present_async(rt2_tracer* tr, const rt2_present_params* p, uint8_t* out_rgba);
RT2_API int rt2_tracer_image_present(rt2_tracer* tr, const rt2_present_params* p, uint8_t* out_rgba);
RT2_API int rt2_tracer_image_move_camera(rt2_tracer* tr, const rt2_camera_desc* cam, const rt2_temporal_params* tp);
RT2_API int rt2_tracer_image_present_time(rt2_tracer* tr, double* ms);
RT2_API int rt2_deinterleave_estimate_host(const float* stacks, const float* stacks2, float* image, float* image_nc,
                                           float* variance, int width, int height, int band_h, int world,
                                           int64_t frames);

/* ---- Adaptive sampling of the gathered image ----
 * Opt-in: a tracer that never calls these allocates nothing new and launches exactly what it launched before.
 * "Adaptive sampling" above for a create_multi or joined tracer, whose gathered image divided by one common frame
 * index: with it on, every rank's stack of sample counts n_p travels with its accumulation (a third transfer of the
 * gather's RCCL group; on one GPU a third copy on the root's stream), and the root's kernel divides each pixel's sum
 * by its own n_p. The calls of that section keep their refusals on these tracers, and a plain tracer switched on
 * by rt2_tracer_enable_adaptive behaves as before, its refusals of gather_estimate, image_resolve, image_present*
 * and image_move_camera included. The check's window runs along the row and partitions hold whole rows, so every
 * decision, every sum and every count is, bit for bit, that of a one-GPU tracer under rt2_tracer_enable_adaptive at
 * the same seed, size, camera and steps.
 * image_enable_adaptive: on a create_multi tracer, enable_adaptive on every part; on a joined tracer, on this rank
 *   (call it after rt2_tracer_join, which refuses an adaptive tracer; every rank calls it); on a plain one-GPU
 *   tracer (world 1) enable_adaptive, and its gathers carry the counts. Needs moments on and the threaded traversal
 *   on every part (asked before any part changes). It synchronises, reallocates, resets the frame index and the
 *   sums, and drops the gathered image and a whole-image history held. on = 0 switches adaptive sampling off the
 *   same way.
 * image_adaptive_check: adaptive_check on every part. On a create_multi tracer every part's check and the copy of
 *   its totals are enqueued before any is waited for, so the checks overlap across the GPUs and the host waits
 *   once per part. `out` is the whole image's: pixels, active, retired, samples and nonfinite summed over the
 *   parts, frames the common FrameIdx(). Collective on joined tracers: every rank calls it; after the local check
 *   its four totals and its pixel count are summed over the ranks on the device (ncclAllReduce, uint64, on the
 *   tracer's stream) before the one copy to the host, so every rank receives the same whole-image scalars, while
 *   what a rank launches next follows its own active count.
 * image_render_adaptive: render_adaptive's loop over image_adaptive_check; it stops when the whole image has no
 *   active pixel. On joined tracers every rank leaves the loop at the same step.
 * image_part_adaptive: the scalars the last check left of GPU `part` alone, before the sum (part 0 of a plain or
 *   joined tracer is itself): how evenly the active pixels stay spread over the parts.
 * image_sample_counts: n_p of the gathered image, uint32 per image pixel, on the root. Blocks. Like the other
 *   rt2_tracer_image_* readbacks it reads what the last gather (or gather_estimate) left.
 * With it on: gather and gather_estimate carry the counts; image_accumulation, image_non_converted_pixels (sum /
 *   (float)n_p), image_pixels and image_variance (from each pixel's own n_p) are those of the one-GPU adaptive
 *   tracer; a create_multi tracer's non_converted_pixels and pixels likewise, its moments and standard_error as
 *   before (the parts' rows placed on the host). image_resolve and image_present* run unchanged, the blend's
 *   length being each pixel's n_p. image_move_camera pushes the blend as the root's history under the camera the
 *   frames were rendered with, then sets the camera and resets every part, which reactivates every pixel.
 * deinterleave_adaptive_host: the CPU statement of that gather's kernel, beside rt2_deinterleave_estimate_host: the
 *   rank-major stacks [world][rt2_band_rows_max][width] of the sums (float3), their squares (float3) and the counts
 *   (uint32) -> image-order sums `image`, means `image_nc` = sum / (float)n_p, `variance` (float) and `image_counts`.
 *   stacks2 and variance may both be NULL (the plain gather). No GPU needed.
 * RT2_ERR_INVALID: image_enable_adaptive(1) with moments off or without the threaded traversal, or on a
 *   set_partition tracer (world > 1) that is not joined; image_adaptive_check, image_render_adaptive,
 *   image_part_adaptive and image_sample_counts with it off; a check with fewer than 2 frames; a window outside
 *   [0, 64] or a threshold that is negative or NaN; a NULL tracer or output; image_part_adaptive with a part out
 *   of range or before the first check since a reset; image_sample_counts before a gather or on a rank other than
 *   0; a gather whose ranks disagree on whether it is on; deinterleave_adaptive_host with a NULL argument (stacks2
 *   and variance excepted, together), a negative size or world < 1. A refused call changes nothing. */
RT2_API int rt2_tracer_image_enable_adaptive(rt2_tracer* tr, int on);
RT2_API int rt2_tracer_image_adaptive_check(rt2_tracer* tr, float threshold, int window, rt2_adaptive* out);
RT2_API int rt2_tracer_image_render_adaptive(rt2_tracer* tr, float threshold, int window, int min_frames, int max_frames,
                                             int check_every, rt2_adaptive* out);
RT2_API int rt2_tracer_image_part_adaptive(rt2_tracer* tr, int part, rt2_adaptive* out);
RT2_API int rt2_tracer_image_sample_counts(rt2_tracer* tr, uint32_t* out); /* n_p per image pixel */
RT2_API int rt2_deinterleave_adaptive_host(const float* stacks, const float* stacks2 /* may be NULL */,
                                           const uint32_t* counts, float* image, float* image_nc,
                                           float* variance /* may be NULL */, uint32_t* image_counts, int width,
                                           int height, int band_h, int world);

/* ---- Ray queries ----
 * Opt-in: a tracer that never calls these allocates nothing new and launches what it launched before.
 * The scene's closest Hit for rays the caller owns (picking, focusing, visibility between two points, feature
 * buffers for a camera of the caller's own), n rays per call, traced by the kernels' traversal: the threaded
 * program where the scene has one, else the stack walk (raytrace2_amd/csrc/query.h holds the layouts and the rule).
 * A ray, 8 floats: ox oy oz tmax | dx dy dz time. The interval is (0.001, tmax); FLT_MAX is "unbounded". The
 *   direction is taken as given, not normalised, so t is in units of |d|, as the reference's Hit sees it.
 * An answer, 16 floats, the feature record's layout: 0 flag: 1 hit, 0 miss, -1 not traced; 1 t (model-space under
 *   a transformed child, the reference's quirk); 2-4 point; 5-7 normal (facing against the ray); 8 front_face; 9
 *   material index; 10-12 albedo by the feature pass's rule: the material table's albedo (metal, lambertian), (1, 1,
 *   1) (dielectric), Texture::Value at the hit (texture, diffuse_light, isotropic); 13 dist = sqrt(dot(point - o,
 *   point - o)); 14-15 0; every operation rounded on its own. A miss: slot 0 = 0, the background in 10-12, every
 *   other slot 0. A ray that was not traced: slot 0 = -1, every other slot 0.
 * A ConstantMedium on the way draws from the path stream (`seed`, pixel 0xFFFFFFF0, frame 0) from its start, the
 *   same for every ray of the call: with the tracer's seed, a normalised pixel-centre ray, tmax FLT_MAX and time 0
 *   the answer is rt2_tracer_features' record of that pixel, bit for bit.
 * query_ray_valid: whether a ray is traced (1) or answered -1 (0): all eight words finite; 0.001 < tmax; 0 <= time
 *   <= 1; every origin coordinate within +-2^64; the largest of |dx|, |dy|, |dz| within [2^-20, 2^20] (so d != 0):
 *   the domain on which the kernels' exact shortcuts are proven. It contains every unit direction and the
 *   un-normalised pixel-centre rays of the shipped scenes' cameras. NULL: 0.
 * intersect: host buffers. It launches queued frames first, as a readback does, copies in, traces and copies out
 *   in chunks of at most RT2_QUERY_CHUNK rays (environment, read at every call, default 2^22, rounded up to a
 *   multiple of 64) through two device buffers the tracer keeps and grows on demand, and synchronises.
 * intersect_device: device pointers on the tracer's device. It only enqueues on the tracer's stream and returns at
 *   once, adds nothing to rt2_stats.host_waits and is complete after rt2_tracer_synchronize or when
 *   rt2_tracer_query returns 1. It does not launch queued frames.
 * occluded, occluded_device: "is anything in the way?" for the same ray records under the same validity rule,
 *   interval (0.001, tmax) and medium stream: one int8_t per ray, 1 occluded, 0 clear, -1 not traced, which is slot
 *   0 of the record intersect writes for that ray and seed, for every valid ray, seed and traversal (the walk is
 *   intersect's up to its first accepted primitive and ends there; nothing is resolved or shaded). The host entry
 *   behaves as intersect (queued frames first, RT2_QUERY_CHUNK, the same two device buffers, one wait) and moves 32
 *   bytes in and 1 byte out per ray; the device entry only enqueues, as intersect_device, and writes exactly n
 *   bytes. Refusals as intersect's.
 * intersect_time: GPU time (HIP events) of the last query's kernels, of either kind: the last intersect,
 *   intersect_device, occluded or occluded_device call (every chunk's, not the copies), in ms; -1 while that
 *   call has not finished, or when there was none. It polls the events and never waits.
 * A call changes no render state: accumulation, moments, counts, FrameIdx(), feature cache and history are
 *   unchanged. It works before on_resize, and on a set_partition or joined tracer (the scene is whole on every
 *   rank and no image is involved). n == 0 is RT2_OK and does nothing.
 * RT2_ERR_INVALID: a NULL tracer or pointer; n < 0 or n >= 2^31; a create_multi tracer; a scene whose stack is
 *   deeper than the kernel's with the threaded traversal off (RT2_NO_LINEAR). A refused call changes nothing. */
RT2_API int rt2_query_ray_valid(const float* ray8);
RT2_API int rt2_tracer_intersect(rt2_tracer* tr, int64_t n, const float* rays, uint64_t seed, float* out);
RT2_API int rt2_tracer_intersect_device(rt2_tracer* tr, int64_t n, const float* d_rays, uint64_t seed, float* d_out);
RT2_API int rt2_tracer_occluded(rt2_tracer* tr, int64_t n, const float* rays, uint64_t seed, int8_t* out);
RT2_API int rt2_tracer_occluded_device(rt2_tracer* tr, int64_t n, const float* d_rays, uint64_t seed, int8_t* d_out);
RT2_API int rt2_tracer_intersect_time(rt2_tracer* tr, double* ms);

/* ---- Ambient occlusion ----
 * Opt-in: a tracer that never calls these allocates nothing new and launches what it launched before.
 * Per point the number of `samples` cosine-weighted occlusion rays that are blocked, one uint32_t per point, drawn
 * and traced on the GPU (raytrace2_amd/csrc/ambient.h holds the rule; the kernel, rt2_ambient_direction and the host
 * test evaluate that one text).
 * A point, 8 floats, the ray record's shape: px py pz tmax | nx ny nz time. It is valid iff rt2_query_ray_valid
 *   holds for these eight words, the normal standing in for the direction. An invalid point answers 0xFFFFFFFF.
 * Sample s of the point with stream index i, every float operation rounded on its own: u = the first RandUnitVec3
 *   draw of the path stream (seed, pixel word i, frame word 0x80000000 + s), above every render frame index; v = n +
 *   u; v = n where every |component of v| <= 1e-8 (Lambertian scatter's guard); d = v * (1 / sqrt((vx vx + vy vy) +
 *   vz vz)). The ray (p, tmax | d, time) is traced exactly as rt2_tracer_occluded traces that record: interval
 *   (0.001, tmax), media drawing from the stream (seed, 0xFFFFFFF0, 0). A built ray that fails rt2_query_ray_valid
 *   is not traced and counts as clear. The count is the number of s in [0, samples) whose answer is 1.
 * ambient_direction: d of the rule from a normal and a unit-vector draw (3 floats each), on the host.
 * ambient (image mode): the points are the tracer's cached feature records (rt2_tracer_features): point = slots 2-4,
 *   normal = slots 5-7, time 0, tmax = radius (FLT_MAX: unbounded); i is the global pixel index y * width + x, so a
 *   set_partition tracer answers what the whole image answers on its rows; a pixel whose ray missed answers
 *   0xFFFFFFFF. One word per local pixel into a host buffer, in rt2_tracer_accumulation's row order. It behaves as a
 *   readback: it launches queued frames, runs the feature pass under `seed` if the cache is stale (the cache is
 *   keyed by camera, size, partition and seed: a seed other than the tracer's makes the next rt2_tracer_features
 *   trace again), and waits once.
 * ambient_device: the same into device memory on the tracer's device, exactly `local pixels` words. It only
 *   enqueues on the tracer's stream, adds nothing to rt2_stats.host_waits and is complete when rt2_tracer_query
 *   returns 1.
 * ambient_points, ambient_points_device (point mode): n caller records, i = the record's index. The host entry goes
 *   in chunks of RT2_QUERY_CHUNK points through the tracer's two query buffers, as occluded does; the device entry
 *   only enqueues and writes exactly n words. They work before on_resize and on set_partition and joined tracers.
 * A launch takes as many samples of every point as keep points x samples below 2^31 and a larger call is split by
 *   sample ranges; counts are integer sums, so the bytes are the same on every run and under every split.
 * ambient_time: GPU time (HIP events) of the last ambient call's kernels in ms (a stale cache's feature pass not
 *   included); -1 while that call has not finished, or when there was none. It polls and never waits.
 * Quirks, the reference's and this rule's: a transformed child compares its model-space t with tmax (occluded's
 *   quirk). Every ray of a call shares the one medium stream, so in a scene wrapped in a medium (book 2's mist) an
 *   image's counts are all 0 or all `samples` around one radius, and the camera's first hits there lie in the mist.
 *   dot(d, n) can be slightly negative where a record's normal is not unit.
 * A call changes no render state: accumulation, moments, counts, FrameIdx() and history are unchanged, and a second
 *   call returns the same bytes. n == 0 is RT2_OK and does nothing.
 * RT2_ERR_INVALID: a NULL tracer or pointer; samples outside [1, 65535]; a radius that is NaN, infinite or <= 0.001;
 *   n < 0 or n >= 2^31; image mode on a tracer without an image (rt2_tracer_create gives every tracer the scene's
 *   default one, as on_resize would) or on a joined tracer; a create_multi tracer; what features
 *   (image mode) and occluded refuse for the scene's stack depth. A refused call changes nothing. */
RT2_API int rt2_ambient_direction(const float* n3, const float* u3, float* d3);
RT2_API int rt2_tracer_ambient(rt2_tracer* tr, int samples, float radius, uint64_t seed, uint32_t* out);
RT2_API int rt2_tracer_ambient_device(rt2_tracer* tr, int samples, float radius, uint64_t seed, uint32_t* d_out);
RT2_API int rt2_tracer_ambient_points(rt2_tracer* tr, int64_t n, const float* points, int samples, uint64_t seed,
                                      uint32_t* out);
RT2_API int rt2_tracer_ambient_points_device(rt2_tracer* tr, int64_t n, const float* d_points, int samples,
                                             uint64_t seed, uint32_t* d_out);
RT2_API int rt2_tracer_ambient_time(rt2_tracer* tr, double* ms);

/* ---- Radiance queries ----
 * Opt-in: a tracer that never calls these allocates nothing new and launches what it launched before.
 * The radiance RayColor returns along rays the caller owns, path-traced on the GPU (raytrace2_amd/csrc/radiance.h
 * holds the rule; the kernels and the host test evaluate that one text).
 * A ray, 8 floats, the ray record of "Ray queries": ox oy oz tmax | dx dy dz time, valid iff rt2_query_ray_valid.
 * Stream words: each ray has two uint32_t (pixel word, frame word), streams[i][0..1]; with streams == NULL they are
 *   (i, 0x40000000), i the ray's index in the call: clear of the render's frame indices and of ambient's
 *   0x80000000 + s.
 * Sample s of ray i, s in [0, samples): open the path stream (seed, pixel word, frame word + s), discard its first
 *   first_draw uniforms, and run RayColorForward for max_depth on the ray. The first segment's interval is (0.001,
 *   tmax), every later one's (0.001, FLT_MAX); the direction is taken as given, as intersect takes it; a
 *   ConstantMedium draws from the sample's own stream, as in a render, not from the probe stream of the other
 *   queries. The sample is thr * emission, thr * background, or 0 when the depth runs out.
 *   With the camera's own ray for pixel (x, y) at frame f (normalised direction, tmax = FLT_MAX), the words (y * width
 *   + x, f), first_draw = 3 (5 with defocus: the draws Camera::GetRay took) and the tracer's seed, a sample is, bit
 *   for bit, that frame's sample of that pixel in a render.
 * out_sum: 3 floats per ray, ((0 + sample_0) + sample_1) + ..., each addition rounded on its own (the render's
 *   accumulation); the caller divides. out_rays (may be NULL): one uint32_t per ray, the rays cast (RayColor entries
 *   with depth > 0) over the samples, the render's ray_counts. An invalid ray answers 0, 0, 0 and 0xFFFFFFFF.
 * rt2_radiance_params (NULL: defaults): samples 1..65535 (1); max_depth 1..65535, 0 = the tracer's (0); first_draw
 *   0..8 (0). frame word + samples must not pass 2^32: the host entry checks its streams and refuses; for the device
 *   entry that is the caller's duty (the frame word wraps).
 * radiance: host pointers. It behaves as intersect: it launches queued frames, goes in chunks of RT2_QUERY_CHUNK
 *   rays through the tracer's query buffers and a slot buffer (16 bytes per (ray, sample) of a launch, at most
 *   RT2_RADIANCE_ITEMS of them, default 2^24 = 256 MiB, at most 2^28; a larger chunk is split by sample ranges, then by ray ranges, and the
 *   ordered sum continues across the ranges, so the split does not show), and waits once.
 * radiance_device: device pointers on the tracer's device; d_streams and d_out_rays may be NULL. It only enqueues on
 *   the tracer's stream, writes exactly n results, adds nothing to rt2_stats.host_waits and is complete when
 *   rt2_tracer_query returns 1.
 * radiance_time: GPU time (HIP events) of the last radiance call's kernels in ms; -1 while that call has not
 *   finished, or when there was none. It polls and never waits.
 * RT2_RADIANCE_REFILL=0 (read at every call) gives every lane exactly one (ray, sample) instead of letting lanes
 *   whose path ended take further ones; the bytes are the same.
 * A call changes no render state and a second call returns the same bytes. n == 0 is RT2_OK and does nothing. The
 *   calls work before on_resize and on set_partition and joined tracers.
 * RT2_ERR_INVALID: samples, max_depth or first_draw out of range; n < 0 or n >= 2^31; a NULL rays, out_sum or
 *   tracer; a frame word that would wrap (host entry); a create_multi tracer; what intersect refuses for the
 *   scene's stack depth. A refused call changes nothing. */
typedef struct {
  int samples;
  int max_depth;
  uint32_t first_draw;
} rt2_radiance_params;
RT2_API void rt2_radiance_defaults(rt2_radiance_params* p);
RT2_API int rt2_tracer_radiance(rt2_tracer* tr, int64_t n, const float* rays, const uint32_t* streams,
                                const rt2_radiance_params* p, uint64_t seed, float* out_sum, uint32_t* out_rays);
RT2_API int rt2_tracer_radiance_device(rt2_tracer* tr, int64_t n, const float* d_rays, const uint32_t* d_streams,
                                       const rt2_radiance_params* p, uint64_t seed, float* d_out_sum,
                                       uint32_t* d_out_rays);
RT2_API int rt2_tracer_radiance_time(rt2_tracer* tr, double* ms);

/* Diagnostic: checks the kernel's exact arithmetic shortcuts against their reference form on n
 * random inputs on `device` (which 0: division by a correctly rounded reciprocal, accepted quad
 * distances; which 1: the NaN-free slab test; which 2: reciprocal and square root without range
 * scaling; which 3: division by a correctly rounded reciprocal over any quotient, numerators down to
 * 2^-100; which 4: the accelerated-list padded slab test culls no box the exact padded slab accepts,
 * zero direction components included; which 5: the reciprocal without range scaling for every float
 * bit pattern below n, n = 2^32 for all of them; which 6: division by a correctly rounded reciprocal
 * for the first n pairs of significands, n = 2^46 for all of them; which 7: the same for every
 * numerator significand against n / 2^23 divisor significands each; which 8: sphere roots by the
 * reciprocal against IEEE division on rays from near a sphere's surface, `checked` = the admitted
 * inputs whose smaller numerator cancelled; which 9: the square root without range scaling at the
 * samplers' inputs for every 24-bit uniform, n = 2^24). Writes the number of mismatches and of inputs checked. */
RT2_API int rt2_selftest(int device, int which, uint64_t n, uint64_t seed, uint64_t* mismatches, uint64_t* checked);

/* ---- util::WriteImage (Util.cpp:39-79): sqrt gamma, clamp(x*255.999), vertical flip ---- */
RT2_API int rt2_write_image(const float* pixels, int width, int height, const char* path, int png);

#ifdef __cplusplus
}
#endif

#endif /* RT2_H_ */
