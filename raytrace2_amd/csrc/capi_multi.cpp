// capi_multi.cpp — the gather of the ranks' row bands to rank 0 and the multi-GPU entry points of include/rt2.h: a
// multi-GPU tracer is a facade over one one-GPU tracer per device.
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "tracer.h"

using namespace rt2;
using namespace rt2::detail;

namespace {

// Row-band height of the multi-GPU partitions (band_h 0). Measured, 8-way split emulated rank by rank
// on one MI355X (job rate = all ranks' rays / the slowest rank's time), band heights 8 / 4 / 2 / 1:
// Cornell 190 / 193 / 197 / 198 k Mray/s, book 1 55.9 / 57.5 / 54.9 / 54.6 k, Cornell volume
// 119.6 / - / 121.5 / 122.4 k, book 2 9.89 / - / 10.15 / 9.81 k. Narrow bands balance the ranks
// (image cost varies smoothly with the row); 2 rows (32x2 work tiles) is within 1-5 % of the best.
constexpr int kDefaultBandH = 2;

// ---- multi-GPU gather ----
// Sizes the root's gathered band stacks and full-image buffers for its current dims and world.
int EnsureImage(rt2_tracer* root) {
  const size_t npix = (size_t)root->width * (size_t)root->height;
  const size_t stacks = (size_t)root->world * (size_t)BandRowsMax(root) * (size_t)root->width * 3 * sizeof(float);
  if (root->d_image.bytes() == npix * 3 * sizeof(float) && root->d_stacks.bytes() == stacks) return RT2_OK;
  FreeImage(root);
  HIP_TRY(hipSetDevice(root->device));
  HIP_TRY(root->d_stacks.Alloc(stacks));
  HIP_TRY(root->d_image.Alloc(npix * 3 * sizeof(float)));
  HIP_TRY(root->d_image_nc.Alloc(npix * 3 * sizeof(float)));
  HIP_TRY(root->d_image_px.Alloc(npix * 4));
  NoteDeviceBytes(root);
  return RT2_OK;
}

// The root's stacks of the gathered sums of squares and the variance plane (rt2_tracer_gather_estimate), sized
// like EnsureImage's buffers, which it runs after (EnsureImage frees these with the image).
int EnsureEstimate(rt2_tracer* root) {
  const size_t npix = (size_t)root->width * (size_t)root->height;
  if (root->d_stacks2.bytes() == root->d_stacks.bytes() && root->d_image_var.bytes() == npix * sizeof(float))
    return RT2_OK;
  HIP_TRY(hipSetDevice(root->device));
  HIP_TRY(root->d_stacks2.Alloc(root->d_stacks.bytes()));
  HIP_TRY(root->d_image_var.Alloc(npix * sizeof(float)));
  NoteDeviceBytes(root);
  return RT2_OK;
}

// The root's stacks of the gathered sample counts and n_p in image order (a gather of ranks with image_adaptive
// on), sized like EnsureImage's buffers, which it runs after (EnsureImage frees these with the image); a root
// whose ranks never switch image_adaptive on allocates neither.
int EnsureCounts(rt2_tracer* root) {
  const size_t npix = (size_t)root->width * (size_t)root->height;
  const size_t stacks = (size_t)root->world * (size_t)BandRowsMax(root) * (size_t)root->width * sizeof(uint32_t);
  if (root->d_stacks_n.bytes() == stacks && root->d_image_n.bytes() == npix * sizeof(uint32_t)) return RT2_OK;
  HIP_TRY(hipSetDevice(root->device));
  HIP_TRY(root->d_stacks_n.Alloc(stacks));
  HIP_TRY(root->d_image_n.Alloc(npix * sizeof(uint32_t)));
  NoteDeviceBytes(root);
  return RT2_OK;
}

// Gathers the band stacks of `ranks` (every rank this thread drives: a multi tracer's parts, or
// one joined tracer) to rank 0 and de-interleaves them there. RCCL unless `loopback` (the ranks
// share one GPU and their stacks are copied on it). Enqueued on the streams; does not wait.
// estimate: the stacks of the sums of squares travel with them (the same RCCL group, or copies on the
// root's stream), and the root's kernel also writes the variance of the mean (rt2_tracer_gather_estimate);
// its refusals come before anything is enqueued. With image_adaptive on (rt2.h "Adaptive sampling of the gathered
// image") every rank's stack of sample counts travels too, as a third transfer of the same group, and the root's
// kernel divides each pixel's sum by its own count; the ranks must agree on it (checked here for the ranks this
// thread drives, before anything is enqueued).
int GatherRanks(const std::vector<rt2_tracer*>& ranks, bool loopback, bool estimate) {
  rt2_tracer* root = nullptr;
  const bool counts = ranks[0]->image_adaptive;
  for (const rt2_tracer* p : ranks)
    if (p->image_adaptive != counts)
      return Fail(RT2_ERR_INVALID, "gather: the ranks disagree on adaptive sampling of the gathered image");
  if (estimate) {
    for (const rt2_tracer* p : ranks) {
      if (p->adaptive_on && !p->image_adaptive)
        return Fail(RT2_ERR_INVALID, "gather_estimate: adaptive sampling is on (the gathered estimate divides by one "
                                     "frame index)");
      if (!p->moments_on) return Fail(RT2_ERR_INVALID, "gather_estimate: moments not enabled (rt2_tracer_enable_moments)");
      if (p->frame_idx + p->queued < 2) return Fail(RT2_ERR_INVALID, "gather_estimate needs at least 2 frames");
      if (!loopback && !p->comm) return Fail(RT2_ERR_INVALID, "gather: tracer is not part of a communicator");
      if (p->width != ranks[0]->width || p->height != ranks[0]->height ||
          p->frame_idx + p->queued != ranks[0]->frame_idx + ranks[0]->queued)
        return Fail(RT2_ERR_INVALID, "gather: the ranks disagree on dims or frame index");
    }
  }
  for (rt2_tracer* p : ranks) {
    int rc = Flush(p);
    if (rc != RT2_OK) return rc;
    if (p->rank == 0) root = p;
  }
  const rt2_tracer* r0 = ranks[0];
  for (rt2_tracer* p : ranks)
    if (p->width != r0->width || p->height != r0->height || p->frame_idx != r0->frame_idx)
      return Fail(RT2_ERR_INVALID, "gather: the ranks disagree on dims or frame index");
  const size_t count = (size_t)BandRowsMax(r0) * (size_t)r0->width * 3;  // floats per rank
  const size_t count_n = count / 3;                                       // sample counts per rank
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (root) {
    int rc = EnsureImage(root);
    if (rc != RT2_OK) return rc;
    if (estimate && (rc = EnsureEstimate(root)) != RT2_OK) return rc;
    if (counts && (rc = EnsureCounts(root)) != RT2_OK) return rc;
    HIP_TRY(hipSetDevice(root->device));
    e0 = TakeEvent(root);
    e1 = TakeEvent(root);
    if (e0) HIP_TRY(hipEventRecord(e0, root->stream));
  }
  if (count > 0) {
    if (loopback) {
      for (rt2_tracer* p : ranks) {
        HIP_TRY(hipSetDevice(p->device));
        if (p != root) {
          hipEvent_t e = TakeEvent(p);
          if (!e) return Fail(RT2_ERR_HIP, "event create failed");
          HIP_TRY(hipEventRecord(e, p->stream));
          HIP_TRY(hipStreamWaitEvent(root->stream, e, 0));
          p->event_pool.push_back(e);
        }
        HIP_TRY(hipMemcpyAsync(root->d_stacks.get<float>() + (size_t)p->rank * count, p->d_accum.get<float>(),
                               count * sizeof(float), hipMemcpyDeviceToDevice, root->stream));
        if (estimate)
          HIP_TRY(hipMemcpyAsync(root->d_stacks2.get<float>() + (size_t)p->rank * count, p->d_moment2.get<float>(),
                                 count * sizeof(float), hipMemcpyDeviceToDevice, root->stream));
        if (counts)  // d_counts is as tall as d_accum (capi.cpp Realloc): the padding rows are there, and zero
          HIP_TRY(hipMemcpyAsync(root->d_stacks_n.get<uint32_t>() + (size_t)p->rank * count_n, p->d_counts.get<uint32_t>(),
                                 count_n * sizeof(uint32_t), hipMemcpyDeviceToDevice, root->stream));
      }
      // later work on a part's stream (Render, Reset) must not overwrite its accumulation (or its sums of
      // squares) while the root's copy may still read it: every part stream waits for all the copies
      if (ranks.size() > 1) {
        HIP_TRY(hipSetDevice(root->device));
        hipEvent_t e = TakeEvent(root);
        if (!e) return Fail(RT2_ERR_HIP, "event create failed");
        HIP_TRY(hipEventRecord(e, root->stream));
        for (rt2_tracer* p : ranks)
          if (p != root) HIP_TRY(hipStreamWaitEvent(p->stream, e, 0));
        root->event_pool.push_back(e);
      }
    } else {
      for (rt2_tracer* p : ranks)
        if (!p->comm) return Fail(RT2_ERR_INVALID, "gather: tracer is not part of a communicator");
      NCCL_TRY(ncclGroupStart());
      for (rt2_tracer* p : ranks) {
        ncclResult_t r = ncclGather(p->d_accum.get<float>(), p == root ? root->d_stacks.get<float>() : nullptr, count,
                                    ncclFloat32, 0, p->comm, p->stream);
        if (r != ncclSuccess) {
          (void)ncclGroupEnd();
          return Fail(RT2_ERR_HIP, std::string("ncclGather: ") + ncclGetErrorString(r));
        }
        if (estimate)
          r = ncclGather(p->d_moment2.get<float>(), p == root ? root->d_stacks2.get<float>() : nullptr, count,
                         ncclFloat32, 0, p->comm, p->stream);
        if (r != ncclSuccess) {
          (void)ncclGroupEnd();
          return Fail(RT2_ERR_HIP, std::string("ncclGather: ") + ncclGetErrorString(r));
        }
        if (counts)
          r = ncclGather(p->d_counts.get<uint32_t>(), p == root ? root->d_stacks_n.get<uint32_t>() : nullptr, count_n,
                         ncclUint32, 0, p->comm, p->stream);
        if (r != ncclSuccess) {
          (void)ncclGroupEnd();
          return Fail(RT2_ERR_HIP, std::string("ncclGather: ") + ncclGetErrorString(r));
        }
      }
      NCCL_TRY(ncclGroupEnd());
    }
  }
  if (root) {
    HIP_TRY(hipSetDevice(root->device));
    if (counts)
      HIP_TRY(LaunchDeinterleaveAdaptive(root->d_stacks.get<float>(), estimate ? root->d_stacks2.get<float>() : nullptr,
                                         root->d_stacks_n.get<uint32_t>(), root->d_image.get<float>(),
                                         root->d_image_nc.get<float>(), root->d_image_px.get<uint8_t>(),
                                         estimate ? root->d_image_var.get<float>() : nullptr,
                                         root->d_image_n.get<uint32_t>(), root->width, root->height, BandH(root),
                                         root->world, BandRowsMax(root), root->stream));
    else if (estimate)
      HIP_TRY(LaunchDeinterleaveEstimate(root->d_stacks.get<float>(), root->d_stacks2.get<float>(),
                                         root->d_image.get<float>(), root->d_image_nc.get<float>(),
                                         root->d_image_px.get<uint8_t>(), root->d_image_var.get<float>(), root->width,
                                         root->height, BandH(root), root->world, BandRowsMax(root), (int)root->frame_idx,
                                         root->stream));
    else
      HIP_TRY(LaunchDeinterleave(root->d_stacks.get<float>(), root->d_image.get<float>(), root->d_image_nc.get<float>(),
                                 root->d_image_px.get<uint8_t>(), root->width, root->height, BandH(root), root->world,
                                 BandRowsMax(root), (int)root->frame_idx, root->stream));
    if (e1) HIP_TRY(hipEventRecord(e1, root->stream));
    if (e0 && e1) root->gpending.emplace_back(e0, e1);
    root->image_frame = root->frame_idx;
    root->image_counts = counts;
    root->gathers++;
  }
  // every rank notes the estimate it took part in (the root's is the one its variance plane holds)
  if (estimate)
    for (rt2_tracer* p : ranks) p->estimate_frame = p->frame_idx;
  return RT2_OK;
}

int GatherAny(rt2_tracer* t, bool estimate) {
  if (IsMulti(t)) return GatherRanks(t->parts, t->loopback, estimate);
  if (t->comm) return GatherRanks({t}, false, estimate);
  if (t->world > 1) return Fail(RT2_ERR_INVALID, "gather: a partitioned tracer must be joined to a communicator");
  return GatherRanks({t}, true, estimate);  // one GPU, whole image: the "gather" is a device-local copy
}
}  // namespace

int rt2::detail::GatherMulti(rt2_tracer* t) { return GatherAny(t, false); }
int rt2::detail::GatherEstimate(rt2_tracer* t) { return GatherAny(t, true); }

int rt2::detail::CurrentEstimate(rt2_tracer* t, bool collective, rt2_tracer** root) {
  rt2_tracer* r = IsMulti(t) ? t->parts[0] : t;
  const bool joined = !IsMulti(t) && t->comm;
  if (r->rank != 0 && !(collective && joined)) return Fail(RT2_ERR_INVALID, "the gathered image lives on rank 0");
  const int64_t cur = r->frame_idx + r->queued;
  if (r->estimate_frame < 0 || r->estimate_frame != cur) {
    if (joined && !collective)
      return Fail(RT2_ERR_INVALID, r->estimate_frame < 0
                                       ? "no gathered estimate (every rank calls rt2_tracer_gather_estimate first)"
                                       : "the gathered estimate is stale: frames were rendered since "
                                         "rt2_tracer_gather_estimate (every rank calls it again)");
    int rc = GatherAny(t, true);
    if (rc != RT2_OK) return rc;
  }
  *root = r;
  return RT2_OK;
}

namespace {
// The root tracer holding the gathered image (rank 0), after a gather.
int ImageRoot(rt2_tracer* t, rt2_tracer** root) {
  rt2_tracer* r = IsMulti(t) ? t->parts[0] : t;
  if (r->rank != 0) return Fail(RT2_ERR_INVALID, "the gathered image lives on rank 0");
  if (r->image_frame < 0) return Fail(RT2_ERR_INVALID, "no gathered image (call rt2_tracer_gather first)");
  int rc = Sync(r);
  if (rc != RT2_OK) return rc;
  *root = r;
  return RT2_OK;
}
}  // namespace

extern "C" {

// ---- multi-GPU entry points ----
int rt2_multi_plan(int n, const int* devices, int band_h, int width, int height, rt2_part_plan* out, int* loopback) {
  if (n < 1 || band_h < 0) return Fail(RT2_ERR_INVALID, "rt2_tracer_create_multi: need n_gpus >= 1, band_h >= 0");
  if (width < 0 || height < 0) return Fail(RT2_ERR_INVALID, "rt2_multi_plan: negative dims");
  std::vector<int> devs((size_t)n);
  for (int i = 0; i < n; i++) devs[(size_t)i] = devices ? devices[i] : i;
  for (int d : devs)
    if (d < 0) return Fail(RT2_ERR_INVALID, "rt2_tracer_create_multi: negative device id");
  const bool all_same = std::all_of(devs.begin(), devs.end(), [&](int d) { return d == devs[0]; });
  std::vector<int> sorted = devs;
  std::sort(sorted.begin(), sorted.end());
  const bool distinct = std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end();
  if (!distinct && !all_same)
    return Fail(RT2_ERR_INVALID, "rt2_tracer_create_multi: devices must be distinct (or all one GPU, for tests)");
  const int bh = band_h > 0 ? band_h : kDefaultBandH;
  if (loopback) *loopback = n > 1 && all_same ? 1 : 0;
  if (out) {
    for (int i = 0; i < n; i++) {
      rt2_part_plan& q = out[i];
      q.device = devs[(size_t)i];
      q.rank = i;
      q.world = n;
      q.band_h = bh;
      q.local_rows = height > 0 ? LocalRows(height, bh, i, n) : 0;
      q.rows_max = rt2::BandRowsMax(height, bh, n);
    }
  }
  return RT2_OK;
}

int rt2_tracer_create_multi(const rt2_scene* s, int n, const int* devices, int band_h, rt2_tracer** out) {
  if (!s || !out) return Fail(RT2_ERR_INVALID, "rt2_tracer_create_multi: null argument");
  *out = nullptr;
  int lb = 0;
  int prc = rt2_multi_plan(n, devices, band_h, 0, 0, nullptr, &lb);
  if (prc != RT2_OK) return prc;
  std::vector<int> devs((size_t)n);
  for (int i = 0; i < n; i++) devs[(size_t)i] = devices ? devices[i] : i;
  auto m = std::make_unique<rt2_tracer>();
  m->loopback = lb != 0;
  const int bh = band_h > 0 ? band_h : kDefaultBandH;
  auto cleanup = [&](int rc) {
    for (rt2_tracer* p : m->parts) rt2_tracer_destroy(p);
    m->parts.clear();
    return rc;
  };
  for (int i = 0; i < n; i++) {
    rt2_tracer* p = nullptr;
    int rc = rt2_tracer_create(s, devs[(size_t)i], &p);
    if (rc != RT2_OK) return cleanup(rc);
    m->parts.push_back(p);
    if ((rc = rt2_tracer_set_partition(p, bh, i, n)) != RT2_OK) return cleanup(rc);
  }
  if (!m->loopback) {  // one communicator per device (rank i on devs[i]), RCCL over xGMI
    std::vector<ncclComm_t> comms((size_t)n, nullptr);
    ncclResult_t r = ncclCommInitAll(comms.data(), n, devs.data());
    if (r != ncclSuccess) return cleanup(Fail(RT2_ERR_HIP, std::string("ncclCommInitAll: ") + ncclGetErrorString(r)));
    for (int i = 0; i < n; i++) m->parts[(size_t)i]->comm = comms[(size_t)i];
  }
  m->device = devs[0];
  m->width = m->parts[0]->width;
  m->height = m->parts[0]->height;
  m->band_h = bh;
  m->world = n;
  *out = m.release();
  return RT2_OK;
}

int rt2_comm_unique_id(uint8_t* out, size_t cap) {
  if (!out || cap < sizeof(ncclUniqueId)) return Fail(RT2_ERR_INVALID, "rt2_comm_unique_id: need RT2_UNIQUE_ID_BYTES");
  ncclUniqueId id;
  NCCL_TRY(ncclGetUniqueId(&id));
  memcpy(out, &id, sizeof(id));
  return RT2_OK;
}

int rt2_tracer_join(rt2_tracer* t, const uint8_t* unique_id, int world, int rank, int band_h) {
  if (!t || !unique_id) return Fail(RT2_ERR_INVALID, "rt2_tracer_join: null argument");
  if (IsMulti(t)) return Fail(RT2_ERR_INVALID, "rt2_tracer_join: a multi-GPU tracer has its own communicators");
  if (t->comm) return Fail(RT2_ERR_INVALID, "rt2_tracer_join: already joined");
  // (also after rt2_tracer_image_enable_adaptive, which is called on the joined tracer: rt2.h)
  if (t->adaptive_on) return Fail(RT2_ERR_INVALID, "rt2_tracer_join: adaptive sampling is on (one-GPU tracers only)");
  int rc = rt2_tracer_set_partition(t, band_h > 0 ? band_h : kDefaultBandH, rank, world);
  if (rc != RT2_OK) return rc;
  ncclUniqueId id;
  memcpy(&id, unique_id, sizeof(id));
  HIP_TRY(hipSetDevice(t->device));
  NCCL_TRY(ncclCommInitRank(&t->comm, world, id, rank));
  return RT2_OK;
}

int rt2_tracer_gather(rt2_tracer* t) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  return GatherMulti(t);
}

int rt2_tracer_image_accumulation(rt2_tracer* t, float* out) {
  if (!t || !out) return Fail(RT2_ERR_INVALID, "null argument");
  rt2_tracer* r = nullptr;
  int rc = ImageRoot(t, &r);
  if (rc != RT2_OK) return rc;
  size_t n = (size_t)r->width * (size_t)r->height;
  if (n) HIP_TRY(hipMemcpy(out, r->d_image.get<float>(), n * 3 * sizeof(float), hipMemcpyDeviceToHost));
  return RT2_OK;
}

// NonConvertedPixels() of the gathered image: accumulation / frame_idx_ (RayTracer.cpp:108-109),
// divided on the GPU by the de-interleave kernel (the same IEEE quotient as the host's)
int rt2_tracer_image_non_converted_pixels(rt2_tracer* t, float* out) {
  if (!t || !out) return Fail(RT2_ERR_INVALID, "null argument");
  rt2_tracer* r = nullptr;
  int rc = ImageRoot(t, &r);
  if (rc != RT2_OK) return rc;
  const size_t n = (size_t)r->width * (size_t)r->height;
  const auto t0 = std::chrono::steady_clock::now();
  if (n) HIP_TRY(hipMemcpy(out, r->d_image_nc.get<float>(), n * 3 * sizeof(float), hipMemcpyDeviceToHost));
  r->readback_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  r->readbacks++;
  return RT2_OK;
}

// The same, enqueued on the root's stream (out: pinned host memory, rt2_host_alloc); complete once
// rt2_tracer_query returns 1 or after rt2_tracer_synchronize. Needs a gather enqueued before it.
int rt2_tracer_image_non_converted_pixels_async(rt2_tracer* t, float* out) {
  if (!t || !out) return Fail(RT2_ERR_INVALID, "null argument");
  rt2_tracer* r = IsMulti(t) ? t->parts[0] : t;
  if (r->rank != 0) return Fail(RT2_ERR_INVALID, "the gathered image lives on rank 0");
  if (r->image_frame < 0) return Fail(RT2_ERR_INVALID, "no gathered image (call rt2_tracer_gather first)");
  HIP_TRY(hipSetDevice(r->device));
  const size_t n = (size_t)r->width * (size_t)r->height;
  hipEvent_t e0 = TakeEvent(r), e1 = TakeEvent(r);
  if (e0) HIP_TRY(hipEventRecord(e0, r->stream));
  if (n) HIP_TRY(hipMemcpyAsync(out, r->d_image_nc.get<float>(), n * 3 * sizeof(float), hipMemcpyDeviceToHost, r->stream));
  if (e1) HIP_TRY(hipEventRecord(e1, r->stream));
  if (e0 && e1) r->rpending.emplace_back(e0, e1);
  r->readbacks++;
  return RT2_OK;
}

int rt2_tracer_image_pixels(rt2_tracer* t, uint8_t* out) {
  if (!t || !out) return Fail(RT2_ERR_INVALID, "null argument");
  rt2_tracer* r = nullptr;
  int rc = ImageRoot(t, &r);
  if (rc != RT2_OK) return rc;
  size_t n = (size_t)r->width * (size_t)r->height;
  if (n) HIP_TRY(hipMemcpy(out, r->d_image_px.get<uint8_t>(), n * 4, hipMemcpyDeviceToHost));
  return RT2_OK;
}

// n_p of the gathered image (rt2.h "Adaptive sampling of the gathered image"): what the gather's kernel wrote in
// image order from the ranks' stacks of counts
int rt2_tracer_image_sample_counts(rt2_tracer* t, uint32_t* out) {
  if (!t || !out) return Fail(RT2_ERR_INVALID, "null argument");
  const rt2_tracer* first = IsMulti(t) ? t->parts[0] : t;
  if (!first->image_adaptive)
    return Fail(RT2_ERR_INVALID, "adaptive sampling of the gathered image not enabled (rt2_tracer_image_enable_adaptive)");
  rt2_tracer* r = nullptr;
  int rc = ImageRoot(t, &r);
  if (rc != RT2_OK) return rc;
  if (!r->image_counts) return Fail(RT2_ERR_INVALID, "no gathered sample counts (call rt2_tracer_gather first)");
  const size_t n = (size_t)r->width * (size_t)r->height;
  if (n) HIP_TRY(hipMemcpy(out, r->d_image_n.get<uint32_t>(), n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RT2_OK;
}

// ---- reconstructing the gathered image (rt2.h): the gather's side; the chain is in capi_filter.cpp ----
int rt2_tracer_gather_estimate(rt2_tracer* t) {
  if (!t) return Fail(RT2_ERR_INVALID, "null tracer");
  return GatherEstimate(t);
}

int rt2_tracer_image_variance(rt2_tracer* t, float* out) {
  if (!t || !out) return Fail(RT2_ERR_INVALID, "null argument");
  rt2_tracer* r = IsMulti(t) ? t->parts[0] : t;
  if (r->rank != 0) return Fail(RT2_ERR_INVALID, "the gathered image lives on rank 0");
  if (r->estimate_frame < 0)
    return Fail(RT2_ERR_INVALID, "no gathered estimate (call rt2_tracer_gather_estimate first)");
  int rc = Sync(r);
  if (rc != RT2_OK) return rc;
  const size_t n = (size_t)r->width * (size_t)r->height;
  if (n) HIP_TRY(hipMemcpy(out, r->d_image_var.get<float>(), n * sizeof(float), hipMemcpyDeviceToHost));
  return RT2_OK;
}

int rt2_deinterleave_estimate_host(const float* stacks, const float* stacks2, float* image, float* image_nc,
                                   float* variance, int width, int height, int band_h, int world, int64_t frames) {
  if (!stacks || !stacks2 || !image || !image_nc || !variance || width < 0 || height < 0 || band_h < 0 || world < 1)
    return Fail(RT2_ERR_INVALID, "bad de-interleave arguments");
  if (frames < 2 || frames > 0x7FFFFFFF) return Fail(RT2_ERR_INVALID, "deinterleave_estimate: need 2 <= frames < 2^31");
  const size_t max_rows = (size_t)rt2::BandRowsMax(height, band_h, world);
  const float fi = (float)frames;
  for (int y = 0; y < height; y++) {
    const BandRow src = BandSource(y, band_h, world);
    for (int x = 0; x < width; x++) {
      const size_t at = 3 * (((size_t)src.rank * max_rows + (size_t)src.row) * (size_t)width + (size_t)x);
      const size_t i = (size_t)y * (size_t)width + (size_t)x;
      const float a[3] = {stacks[at], stacks[at + 1], stacks[at + 2]};
      const float q[3] = {stacks2[at], stacks2[at + 1], stacks2[at + 2]};
      for (int c = 0; c < 3; c++) {
        image[3 * i + c] = a[c];
        image_nc[3 * i + c] = a[c] / fi;
      }
      variance[i] = DenoiseVarianceOfSem(NoiseOfPixel(a, q, frames).sem);
    }
  }
  return RT2_OK;
}

int rt2_deinterleave_adaptive_host(const float* stacks, const float* stacks2, const uint32_t* counts, float* image,
                                   float* image_nc, float* variance, uint32_t* image_counts, int width, int height,
                                   int band_h, int world) {
  if (!stacks || !counts || !image || !image_nc || !image_counts || width < 0 || height < 0 || band_h < 0 || world < 1)
    return Fail(RT2_ERR_INVALID, "bad de-interleave arguments");
  if ((stacks2 == nullptr) != (variance == nullptr))
    return Fail(RT2_ERR_INVALID, "deinterleave_adaptive: stacks2 and variance come together, or both NULL");
  const size_t max_rows = (size_t)rt2::BandRowsMax(height, band_h, world);
  for (int y = 0; y < height; y++) {
    const BandRow src = BandSource(y, band_h, world);
    for (int x = 0; x < width; x++) {
      const size_t from = ((size_t)src.rank * max_rows + (size_t)src.row) * (size_t)width + (size_t)x;
      const size_t i = (size_t)y * (size_t)width + (size_t)x;
      const uint32_t n = counts[from];
      const float fn = (float)n;
      const float a[3] = {stacks[3 * from], stacks[3 * from + 1], stacks[3 * from + 2]};
      for (int c = 0; c < 3; c++) {
        image[3 * i + c] = a[c];
        image_nc[3 * i + c] = a[c] / fn;
      }
      image_counts[i] = n;
      if (variance) {
        const float q[3] = {stacks2[3 * from], stacks2[3 * from + 1], stacks2[3 * from + 2]};
        variance[i] = DenoiseVarianceOfSem(NoiseOfPixel(a, q, (int64_t)n).sem);
      }
    }
  }
  return RT2_OK;
}
}  // extern "C"
