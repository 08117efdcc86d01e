#!/usr/bin/env python3
"""What a temporal resolve costs on one GPU: Cornell 1024^2, 64 frames, push, a small camera move, Reset,
8 frames, then resolves.

Measured with the library's own HIP events on the tracer's stream (rt2_tracer_temporal_time: the resolve's
temporal kernels, the inputs kernel and the blend, without the feature pass, the filter and the readback):
`--reps` resolves after the first (at least ten), without and with the filter, alternated; the first call of
each is reported apart and the median and min-max taken over the rest. The filter's own time is not part of
it (tools/denoise_cost.py measures that call). Beside the times: the bytes a
resolve must move at least (every plane read or written once; each old pixel is wanted by about four taps, which
are cache hits at best) and the time those bytes take at the HBM peak.
Writes one JSON line to --out (default profiles/temporal_cost.json) and prints it."""
import argparse
import dataclasses
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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
ap.add_argument("--denoise-ms", type=float, default=0.795, help="the denoise call to compare with (DESIGN.md §6e)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_cost.json"))
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
tr.set_camera(cam)
tr.Render(a.frames)
tr.temporal_push()
tr.set_camera(dataclasses.replace(cam, center=(cam.center[0] + a.move, cam.center[1] + a.move, cam.center[2])))
tr.Reset()
tr.Render(a.frames_after)
tr.synchronize()

runs = {"plain": [], "denoise": []}
found = None
for i in range(a.reps + 1):
    for kind in ("plain", "denoise"):  # alternated
        out = tr.temporal_resolve(denoise=kind == "denoise", length=True)
        runs[kind].append(tr.temporal_time())
        if found is None:
            found = float((out[1] > a.frames_after).mean())
peak = tr.stats()["device_bytes_peak"]
tr.close()

# per pixel: inputs (24 in, 16 out); blend: colour and variance 16 in and 16 out, the feature record 64 in, the
# history's four words 64 in (each old pixel once), the length 4 out
bytes_inputs = npix * (24 + 16)
bytes_blend = npix * (16 + 64 + 64 + 16 + 4)
bytes_call = bytes_inputs + bytes_blend
bytes_tap_requests = npix * 4 * 64  # what the blend asks of the cache hierarchy


def summary(ms):
    rest = ms[1:]
    return {"first_ms": round(ms[0], 4), "median_ms": round(statistics.median(rest), 4), "min_ms": round(min(rest), 4),
            "max_ms": round(max(rest), 4), "calls": len(rest)}


floor_ms = bytes_call / (a.hbm_peak_gbs * 1e9) * 1e3
plain, den = summary(runs["plain"]), summary(runs["denoise"])
line = json.dumps({"temporal_cost": {
    "workload": f"{a.scene} {w}x{h}: {a.frames} frames, push, centre +{a.move} in x and y, reset, {a.frames_after} frames",
    "params": R.temporal_defaults(), "history_found_fraction": round(found, 4),
    "resolve": plain, "resolve_with_denoise": den,
    "bytes_inputs_min": bytes_inputs, "bytes_blend_min": bytes_blend, "bytes_per_call_min": bytes_call,
    "bytes_tap_requests": bytes_tap_requests, "history_bytes": npix * 64, "device_bytes_peak": peak,
    "hbm_peak_gbs": a.hbm_peak_gbs, "hbm_floor_ms": round(floor_ms, 4),
    "floor_fraction": round(floor_ms / plain["median_ms"], 4),
    "denoise_call_ms": a.denoise_ms, "resolve_over_denoise_call": round(plain["median_ms"] / a.denoise_ms, 4)}})
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write(line + "\n")
print(line, flush=True)
