#!/usr/bin/env python3
"""What showing a reconstructed frame costs on one GPU: Cornell 1024^2, 64 frames, a history pushed, a small
camera move, 8 frames, then the two routes to RGBA8, alternated, `--reps` calls after the first (at least ten):

  (a) today's: temporal_resolve(denoise=True), a blocking float32 readback to pageable memory, then the tone
      map in numpy on the host: wall time per frame;
  (b) present_async into pinned memory: the host time of the call (the enqueue), the wall time until query()
      returns 1, and the GPU time of the present's kernels (rt2_tracer_present_time: inputs, blend, filter, tone map).

The tone-map kernel alone is taken by difference: present(temporal=0, denoise=1)'s kernels (inputs, filter, tone
map) against denoise()'s (inputs, filter), both from HIP events on the tracer's stream; its byte floor is 12 bytes
in and 4 out per pixel at the HBM peak. Last, a ProgressiveLoop at a 16 ms budget over --loop-frames frames
with and without reconstruct={} (moments on in both): ticks, frames per tick and wall time.
Writes one JSON line to --out (default profiles/present_cost.json) and prints it."""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401

import raytrace2_amd as R  # noqa: E402
from raytrace2_amd.progressive import PinnedBuffer, ProgressiveLoop  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scene", default="cornell_box_original.json")
ap.add_argument("--size", default="1024x1024")
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--frames-after", type=int, default=8)
ap.add_argument("--move", type=float, default=20.0, help="added to the camera centre's x and y")
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--loop-frames", type=int, default=512)
ap.add_argument("--budget-ms", type=float, default=16.0)
ap.add_argument("--hbm-peak-gbs", type=float, default=8000.0, help="MI355X HBM3E peak, GB/s")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "present_cost.json"))
a = ap.parse_args()
if a.reps < 10:
    ap.error("--reps must be at least 10")

w, h = (int(v) for v in a.size.split("x"))
npix = w * h
sc = R.Scene(os.path.join(ROOT, "scenes", a.scene), R.DEFAULT_SEED)
tr = R.RayTracer(sc, 0)
tr.SetSamplesPerPixel(a.frames)
tr.OnResize((w, h))
tr.enable_moments()
cam = tr.get_camera()
moved = dataclasses.replace(cam, center=(cam.center[0] + a.move, cam.center[1] + a.move, cam.center[2]))
tr.set_camera(cam)
tr.Render(a.frames)
tr.synchronize()
tr.move_camera(moved)
tr.Render(a.frames_after)
tr.synchronize()
buf = PinnedBuffer((h, w, 4))


def tone_map(c):  # the host's Pixels() arithmetic (tests/present_ref.py)
    v = np.where(c > 0, c, np.float32(0))
    v = np.where(v < 1, v, np.float32(1))
    out = np.full(c.shape[:-1] + (4,), 255, np.uint8)
    out[..., :3] = np.floor(v.astype(np.float64) * 255.999).astype(np.uint8)
    return out


runs = {k: [] for k in ("a_wall", "a_readback", "b_enqueue", "b_wall", "b_gpu", "filter_present_gpu", "denoise_gpu")}
same = None
for i in range(a.reps + 1):  # the routes alternated
    t0 = time.perf_counter()
    c = tr.temporal_resolve(denoise=True)
    t1 = time.perf_counter()
    px_a = tone_map(c)
    t2 = time.perf_counter()
    runs["a_wall"].append((t2 - t0) * 1e3)
    runs["a_readback"].append((t1 - t0) * 1e3)
    t0 = time.perf_counter()
    tr.present_async(buf.array)
    t1 = time.perf_counter()
    while tr.query() != 1:
        pass
    t2 = time.perf_counter()
    runs["b_enqueue"].append((t1 - t0) * 1e3)
    runs["b_wall"].append((t2 - t0) * 1e3)
    runs["b_gpu"].append(tr.present_time())
    if same is None:
        same = bool(np.array_equal(px_a, buf.array))
    # the tone map by difference: (inputs, filter, tone map) against (inputs, filter)
    tr.present_async(buf.array, temporal=0)
    tr.synchronize()
    runs["filter_present_gpu"].append(tr.present_time())
    tr.denoise()
    runs["denoise_gpu"].append(tr.denoise_times()["denoise_ms"])


def summary(ms):
    rest = ms[1:]
    return {"first_ms": round(ms[0], 4), "median_ms": round(statistics.median(rest), 4), "min_ms": round(min(rest), 4),
            "max_ms": round(max(rest), 4), "calls": len(rest)}


def loop_run(reconstruct):
    tr.temporal_clear()
    tr.Reset()
    tr.synchronize()
    loop = ProgressiveLoop(tr, a.loop_frames, budget_ms=a.budget_ms, reconstruct=reconstruct)
    t0 = time.perf_counter()
    loop.run()
    wall = (time.perf_counter() - t0) * 1e3
    ticks = loop.ticks
    loop.close()
    return {"ticks": ticks, "frames_per_tick": round(a.loop_frames / ticks, 2), "wall_ms": round(wall, 2),
            "wall_ms_per_tick": round(wall / ticks, 3)}


loop_run(None)  # warm-up (sample buffers at the loop's sizes)
loops = {"plain": [], "reconstruct": []}
for _ in range(3):  # alternated
    loops["plain"].append(loop_run(None))
    loops["reconstruct"].append(loop_run({}))
tr.close()
buf.close()

s = {k: summary(v) for k, v in runs.items()}
tone_ms = s["filter_present_gpu"]["median_ms"] - s["denoise_gpu"]["median_ms"]
bytes_tone = npix * (12 + 4)
floor_ms = bytes_tone / (a.hbm_peak_gbs * 1e9) * 1e3
line = json.dumps({"present_cost": {
    "workload": f"{a.scene} {w}x{h}: {a.frames} frames, move_camera (centre +{a.move} in x and y), {a.frames_after} frames",
    "routes_agree_byte_for_byte": same,
    "route_a_resolve_plus_numpy_wall": s["a_wall"], "route_a_readback_alone": s["a_readback"],
    "route_b_enqueue_host": s["b_enqueue"], "route_b_wall_until_query": s["b_wall"], "route_b_present_time_gpu": s["b_gpu"],
    "present_filter_only_gpu": s["filter_present_gpu"], "denoise_call_gpu": s["denoise_gpu"],
    "tone_map_by_difference_ms": round(tone_ms, 4), "tone_map_bytes_min": bytes_tone, "hbm_peak_gbs": a.hbm_peak_gbs,
    "tone_map_hbm_floor_ms": round(floor_ms, 5),
    "tone_map_floor_fraction": round(floor_ms / tone_ms, 4) if tone_ms > 0 else None,
    "progressive_loop": {"frames": a.loop_frames, "budget_ms": a.budget_ms, **loops}}})
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write(line + "\n")
print(line, flush=True)
