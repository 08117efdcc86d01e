#!/usr/bin/env python3
"""What an ambient-occlusion image costs on one GPU next to the path a caller had before it (rt2.h "Ambient
occlusion"): Cornell and book 1, 1024^2 pixels, 16 samples per pixel.

Per round, alternated:
  - ambient:  the image call by its device entry (rt2_tracer_ambient_device) into a CUDA tensor, timed with the
              library's own HIP events around its kernels (rt2_tracer_ambient_time); the feature cache is warm;
  - occluded: the caller's path: from the features() read back once, pixels x samples ray records (32 bytes each) are
              built on the host in numpy (cosine-weighted about the normal by the rule's own expression, n + u
              normalised, u from numpy's generator: the same distribution of rays, not the same bits, since the
              rule's Philox stream has no vectorised host form), uploaded, sent through RayTracer.occluded's device
              entry (timed by rt2_tracer_intersect_time: the parent's own kernel) and summed per pixel on the device.
              The host build and the upload are timed separately, by the wall clock around each.
One warm-up round, then `--reps` rounds; medians, with min and max as the run-to-run spread; the ratios
occluded kernel / ambient kernel and (build + upload + occluded kernel) / ambient kernel of the medians with the
range the spreads allow. The mean visibility of both paths is recorded so that a reader sees they drew the same
distribution. Writes one JSON document to --out (default profiles/ambient_cost.json) and prints it."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import raytrace2_amd as R  # noqa: E402

SCENES = {"cornell": ("cornell_box_original.json", 100.0), "book1": ("final_render_book_1.json", 2.0)}

ap = argparse.ArgumentParser()
ap.add_argument("--size", default="1024x1024")
ap.add_argument("--samples", type=int, default=16)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ambient_cost.json"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("ambient_cost: needs a GPU")
w, h = (int(v) for v in a.size.split("x"))
n, k = w * h, a.samples
F32 = np.float32
INVALID = 0xFFFFFFFF


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "calls": len(v)}


def build_rays(feats, radius, rng):
    """pixels x samples ray records from feature records by the rule's expression; a miss pixel's rays are zeros
    (not traced)."""
    f = feats.reshape(-1, 16)
    u01 = rng.random((n, k, 2), dtype=F32)
    z = F32(1) - F32(2) * u01[..., 0]
    r = np.sqrt(F32(1) - z * z)
    phi = F32(2 * np.pi) * u01[..., 1]
    v = f[:, None, 5:8] + np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=-1)
    v = np.where((np.abs(v) <= F32(1e-8)).all(-1, keepdims=True), f[:, None, 5:8], v)  # (the rule's guard)
    v[f[:, 0] == 0] = 1  # (a miss pixel: no normal; its rays are zeroed below)
    v *= (F32(1) / np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]))[..., None]
    rays = np.zeros((n, k, 8), F32)
    rays[..., 0:3] = f[:, None, 2:5]
    rays[..., 3] = F32(radius)
    rays[..., 4:7] = v
    rays[f[:, 0] == 0] = 0
    return rays.reshape(-1, 8)


doc = {"pixels": n, "samples": k, "rays_per_call": n * k, "size": [w, h], "reps": a.reps,
       "version": R.lib.rt2_version().decode(), "scenes": {}}
for key, (fname, radius) in SCENES.items():
    sc = R.Scene(os.path.join(ROOT, "scenes", fname), R.DEFAULT_SEED)
    tr = R.RayTracer(sc, 0)
    tr.OnResize((w, h))
    t0 = time.perf_counter()
    feats = tr.features()
    features_readback_ms = (time.perf_counter() - t0) * 1e3
    hit = feats.reshape(-1, 16)[:, 0] != 0
    rng = np.random.default_rng(11)
    d_counts = torch.empty((n,), dtype=torch.int32, device="cuda")
    times = {"ambient_kernel": [], "occluded_kernel": [], "host_build": [], "upload": [], "device_sum": []}
    vis = {}
    for rep in range(a.reps + 1):  # round 0 warms up
        torch.cuda.synchronize()
        R._native.check(R.lib.rt2_tracer_ambient_device(tr._h, k, radius, R.DEFAULT_SEED, ctypes.c_void_p(d_counts.data_ptr())))
        tr.synchronize()
        amb_ms = tr.ambient_time()
        t0 = time.perf_counter()
        rays = build_rays(feats, radius, rng)
        t1 = time.perf_counter()
        d_rays = torch.from_numpy(rays).cuda()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        occ = tr.occluded(d_rays)
        occ_ms = tr.intersect_time()
        t3 = time.perf_counter()
        sums = (occ == 1).view(n, k).sum(-1)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        if rep == 0:
            c = d_counts.cpu().numpy().view(np.uint32)
            if not np.array_equal(c == INVALID, ~hit) or (c[hit] > k).any():
                sys.exit(f"ambient_cost: {key}: the image call's miss pixels are not features()'s")
            vis = {"hit_pixels": int(hit.sum()),
                   "ambient_mean_visibility": round(float(1 - c[hit].mean() / k), 4),
                   "occluded_mean_visibility": round(float(1 - sums.cpu().numpy()[hit].mean() / k), 4)}
        else:
            times["ambient_kernel"].append(amb_ms)
            times["occluded_kernel"].append(occ_ms)
            times["host_build"].append((t1 - t0) * 1e3)
            times["upload"].append((t2 - t1) * 1e3)
            times["device_sum"].append((t4 - t3) * 1e3)
        del d_rays, occ, rays
    tr.close()
    s = {name: summary(v) for name, v in times.items()}
    am, oc = s["ambient_kernel"], s["occluded_kernel"]
    whole = {m: oc[m] + s["host_build"][m] + s["upload"][m] for m in ("median_ms", "min_ms", "max_ms")}
    doc["scenes"][key] = {
        "scene": fname, "radius": radius, **vis, "features_readback_ms": round(features_readback_ms, 3), **s,
        "ray_bytes": n * k * 32, "mray_s_ambient": round(n * k / am["median_ms"] / 1e3, 1),
        "mray_s_occluded": round(n * k / oc["median_ms"] / 1e3, 1),
        "occluded_kernel_over_ambient_kernel": round(oc["median_ms"] / am["median_ms"], 3),
        "kernel_ratio_min": round(oc["min_ms"] / am["max_ms"], 3), "kernel_ratio_max": round(oc["max_ms"] / am["min_ms"], 3),
        "caller_path_over_ambient_kernel": round(whole["median_ms"] / am["median_ms"], 2),
        "caller_path_ratio_min": round(whole["min_ms"] / am["max_ms"], 2),
        "caller_path_ratio_max": round(whole["max_ms"] / am["min_ms"], 2)}
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print(json.dumps(doc))
