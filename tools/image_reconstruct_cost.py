#!/usr/bin/env python3
"""What reconstructing the gathered image costs on the root, on one MI355X: Cornell 1024^2, 64 frames, moments on,
tracers over devices=[0] (RCCL, a communicator of size 1) and devices=[0] * 4 (four partitions on one GPU,
device-local copies). `--reps` calls after the first (at least ten), the variants alternated:

  (a) gather() against gather_estimate(): GPU time between the HIP events the library records on the root's stream
      around each gather (rt2_stats.gather_ms: the transfers and the root's kernel);
  (b) image_present() on the four-partition tracer against present() on a one-GPU tracer in the same session, after
      the same camera move with a history held: image_present_time() against present_time() (inputs, blend, filter,
      tone map), and whether the two pictures agree byte for byte;
  (c) the gather's kernels alone, from a kernel trace taken in a run of its own:
        rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/image_reconstruct_cost.py --kernels-only
      and then --kernel-stats DIR/.../run_kernel_stats.csv on the measuring run: deinterleave_estimate_kernel against
      its byte floor (24 bytes read and 32 written per pixel at the HBM peak) and against deinterleave_kernel.

Nothing here runs on more than one physical GPU: what the second ncclGather costs over xGMI is not measured.
Writes one JSON line to --out (default profiles/image_reconstruct_cost.json) and prints it."""
import argparse
import csv
import dataclasses
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401

import raytrace2_amd as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scene", default="cornell_box_original.json")
ap.add_argument("--size", default="1024x1024")
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--frames-after", type=int, default=8)
ap.add_argument("--move", type=float, default=20.0, help="added to the camera centre's x and y")
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--hbm-peak-gbs", type=float, default=8000.0, help="MI355X HBM3E peak, GB/s")
ap.add_argument("--kernels-only", action="store_true", help="only the alternated gathers (the run to trace); writes nothing")
ap.add_argument("--kernel-stats", default=None, help="rocprofv3 kernel stats CSV of a --kernels-only run")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_reconstruct_cost.json"))
a = ap.parse_args()
if a.reps < 10:
    ap.error("--reps must be at least 10")

w, h = (int(v) for v in a.size.split("x"))
npix = w * h
sc = R.Scene(os.path.join(ROOT, "scenes", a.scene), R.DEFAULT_SEED)


def tracer(**kw):
    tr = R.RayTracer(sc, 0, **kw)
    tr.SetSamplesPerPixel(a.frames)
    tr.OnResize((w, h))
    tr.enable_moments()
    tr.set_camera(tr.get_camera())
    tr.Render(a.frames)
    tr.synchronize()
    return tr


def summary(ms):
    rest = ms[1:]
    return {"first_ms": round(ms[0], 4), "median_ms": round(statistics.median(rest), 4), "min_ms": round(min(rest), 4),
            "max_ms": round(max(rest), 4), "calls": len(rest)}


def gather_ms(tr, call):
    """GPU ms of one gather, from the library's events on the root's stream."""
    g0 = tr.stats()["gather_ms"]
    call()
    tr.synchronize()
    return tr.stats()["gather_ms"] - g0


tracers = {"rccl_1": tracer(devices=[0]), "loopback_4": tracer(devices=[0] * 4)}
gathers = {}
for name, tr in tracers.items():
    runs = {"gather": [], "gather_estimate": []}
    for _ in range(a.reps + 1):  # alternated
        runs["gather"].append(gather_ms(tr, tr.gather))
        runs["gather_estimate"].append(gather_ms(tr, tr.gather_estimate))
    gathers[name] = {k: summary(v) for k, v in runs.items()}
    gathers[name]["estimate_over_gather"] = round(gathers[name]["gather_estimate"]["median_ms"] /
                                                  gathers[name]["gather"]["median_ms"], 3)
if a.kernels_only:
    for tr in tracers.values():
        tr.close()
    sys.exit(0)
tracers.pop("rccl_1").close()

# (b) the present chain over the gathered image against a one-GPU tracer's, a history held on both
multi = tracers.pop("loopback_4")
plain = tracer()
cam = plain.get_camera()
moved = dataclasses.replace(cam, center=(cam.center[0] + a.move, cam.center[1] + a.move, cam.center[2]))
plain.move_camera(moved)
multi.image_move_camera(moved)
for tr in (plain, multi):
    tr.Render(a.frames_after)
    tr.synchronize()
runs = {"present_time": [], "image_present_time": []}
same = None
for _ in range(a.reps + 1):  # alternated
    px = plain.present()
    plain.synchronize()
    runs["present_time"].append(plain.present_time())
    ipx = multi.image_present()
    multi.synchronize()
    runs["image_present_time"].append(multi.image_present_time())
    if same is None:
        same = bool(np.array_equal(px, ipx))
present = {k: summary(v) for k, v in runs.items()}
plain.close()
multi.close()

# (c) the kernels alone, from the trace of a --kernels-only run
bytes_min = npix * (24 + 32)
floor_ms = bytes_min / (a.hbm_peak_gbs * 1e9) * 1e3
kernels = None
if a.kernel_stats:
    kernels = {}
    for row in csv.DictReader(open(a.kernel_stats)):
        for k in ("deinterleave_estimate_kernel", "deinterleave_kernel"):
            if f"::{k}(" in row["Name"]:
                kernels[k] = {"calls": int(row["Calls"]), "average_ms": round(float(row["AverageNs"]) / 1e6, 5),
                              "min_ms": round(float(row["MinNs"]) / 1e6, 5), "max_ms": round(float(row["MaxNs"]) / 1e6, 5)}
    est = kernels.get("deinterleave_estimate_kernel")
    if est:
        est["floor_fraction"] = round(floor_ms / est["average_ms"], 4)
        est["achieved_gbs"] = round(bytes_min / (est["average_ms"] * 1e-3) / 1e9, 1)

line = json.dumps({"image_reconstruct_cost": {
    "workload": f"{a.scene} {w}x{h}: {a.frames} frames, moments on; presents after image_move_camera (centre +{a.move} "
                f"in x and y) and {a.frames_after} frames",
    "physical_gpus": 1, "not_measured": "more than one physical GPU: the second ncclGather over xGMI, joined world > 1",
    "gather_gpu_ms": gathers, "pictures_agree_byte_for_byte": same, "present_gpu_ms": present,
    "estimate_kernel_bytes_min": bytes_min, "hbm_peak_gbs": a.hbm_peak_gbs,
    "estimate_kernel_hbm_floor_ms": round(floor_ms, 5), "kernel_trace": kernels}})
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write(line + "\n")
print(line, flush=True)
