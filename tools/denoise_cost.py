#!/usr/bin/env python3
"""What the feature pass and the denoiser cost on one GPU: Cornell 1024^2 after 64 frames by default.

Measured with the library's own HIP events on the tracer's stream (rt2_tracer_denoise_times: the feature
kernel alone; the denoise call's kernels from the inputs kernel to the unpack, without the readback):
  - the feature pass, traced again for every call by moving the seed (Cornell has no medium: same records);
  - one denoise call at the defaults, the small steps' tiles staged in LDS (RT2_DENOISE_LDS=1);
  - the same with the LDS path off (RT2_DENOISE_LDS=0),
the two denoise variants alternated, `--reps` calls each (at least ten), the first call of each reported apart
and the median taken over the rest. Beside the times: the bytes every call must move at least (each plane
read or written once per kernel; taps beyond that are cache hits at best) and the time those bytes take at
the HBM peak, so the times can be read against the memory floor.
Writes one JSON line to --out (default profiles/denoise_cost.json) and prints it."""
import argparse
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
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--hbm-peak-gbs", type=float, default=8000.0, help="MI355X HBM3E peak, GB/s")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_cost.json"))
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
tr.Render(a.frames)
tr.synchronize()
defaults = R.denoise_defaults()

feature_ms = []
for i in range(a.reps + 1):
    tr.set_seed(R.DEFAULT_SEED + 1 + i)  # drops the cached buffer; frames are already rendered
    tr.features()
    feature_ms.append(tr.denoise_times()["features_ms"])

runs = {"1": [], "0": []}
for i in range(a.reps + 1):
    for lds in ("1", "0"):  # alternated
        os.environ["RT2_DENOISE_LDS"] = lds
        tr.denoise()
        runs[lds].append(tr.denoise_times()["denoise_ms"])
os.environ.pop("RT2_DENOISE_LDS", None)
tr.close()

it = defaults["iterations"]
# per pixel: inputs (24 in, 16 out), pack (16 + 64 in, 64 out), per pass vbar (32 in, 4 out) and the pass
# (64 + 4 in, 16 out), unpack (16 in, 16 out)
bytes_fixed = npix * (24 + 16 + 16 + 64 + 64 + 16 + 16)
bytes_pass = npix * (32 + 4 + 64 + 4 + 16)
bytes_call = bytes_fixed + it * bytes_pass
bytes_tap_requests = npix * 25 * 64  # what a pass asks of the cache hierarchy


def summary(ms):
    rest = ms[1:]
    return {"first_ms": round(ms[0], 4), "median_ms": round(statistics.median(rest), 4), "min_ms": round(min(rest), 4),
            "max_ms": round(max(rest), 4), "calls": len(rest)}


floor_ms = bytes_call / (a.hbm_peak_gbs * 1e9) * 1e3
lds, direct = summary(runs["1"]), summary(runs["0"])
line = json.dumps({"denoise_cost": {
    "workload": f"{a.scene} {w}x{h} after {a.frames} frames", "params": defaults,
    "features": summary(feature_ms), "features_bytes_written": npix * 64,
    "denoise_lds": lds, "denoise_direct": direct,
    "lds_over_direct": round(lds["median_ms"] / direct["median_ms"], 4),
    "bytes_per_pass_min": bytes_pass, "bytes_per_call_min": bytes_call, "bytes_per_pass_tap_requests": bytes_tap_requests,
    "hbm_peak_gbs": a.hbm_peak_gbs, "hbm_floor_ms": round(floor_ms, 4),
    "floor_fraction_lds": round(floor_ms / lds["median_ms"], 4),
    "floor_fraction_direct": round(floor_ms / direct["median_ms"], 4)}})
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write(line + "\n")
print(line, flush=True)
