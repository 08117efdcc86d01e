#!/usr/bin/env python3
"""What a ray query costs on one GPU (rt2.h "Ray queries"): Cornell and book 1, 1024^2 rays per call.

Three orderings of rays through the device entry (RayTracer.intersect on a CUDA tensor: no copies in the time),
timed with the library's own HIP events around the query kernel (rt2_tracer_intersect_time):
  - coherent: the un-normalised pixel-centre rays pc - center of the scene's camera, in image order;
  - permuted: the same rays in one fixed random permutation (a wave's lanes at unrelated places of the program);
  - random:   unit directions from random points in the scene's box;
next to the feature pass (rt2_tracer_denoise_times: features_kernel, the stack walk over the same pixel-centre
rays, normalised), traced again for every repetition by moving the seed. One warm-up round, then `--reps`
alternated rounds (feature pass, coherent, permuted, random); medians, with min and max as the run-to-run spread.
Writes one JSON document to --out (default profiles/intersect_cost.json) and prints it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import raytrace2_amd as R  # noqa: E402

# (scene file, the box random origins are drawn from: lo, hi)
SCENES = {"cornell": ("cornell_box_original.json", (0.0, 0.0, 0.0), (555.0, 555.0, 555.0)),
          "book1": ("final_render_book_1.json", (-11.0, 0.0, -11.0), (11.0, 3.0, 11.0))}

ap = argparse.ArgumentParser()
ap.add_argument("--size", default="1024x1024")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intersect_cost.json"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("intersect_cost: needs a GPU")
w, h = (int(v) for v in a.size.split("x"))
n = w * h
F32 = np.float32
FLT_MAX = np.finfo(F32).max


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "mray_s": round(n / statistics.median(ms) / 1e3, 1), "calls": len(ms)}


doc = {"rays_per_call": n, "size": [w, h], "reps": a.reps, "version": R.lib.rt2_version().decode(), "scenes": {}}
for key, (fname, lo, hi) in SCENES.items():
    sc = R.Scene(os.path.join(ROOT, "scenes", fname), R.DEFAULT_SEED)
    tr = R.RayTracer(sc, 0)
    tr.SetSamplesPerPixel(16)
    tr.OnResize((w, h))
    cp = sc.camera_params(w, h, 16)
    p00, du, dv, c = cp[0:3], cp[3:6], cp[6:9], cp[9:12]
    x = np.arange(w).astype(F32)[None, :, None]
    y = np.arange(h).astype(F32)[:, None, None]
    pc = (p00 + x * du) + y * dv
    rays = np.zeros((n, 8), F32)
    rays[:, 0:3] = c
    rays[:, 3] = FLT_MAX
    rays[:, 4:7] = (pc - c).reshape(-1, 3)
    rng = np.random.default_rng(7)
    perm = rng.permutation(n)
    rnd = np.zeros((n, 8), F32)
    rnd[:, 0:3] = rng.uniform(lo, hi, (n, 3)).astype(F32)
    rnd[:, 3] = FLT_MAX
    v = rng.normal(size=(n, 3))
    rnd[:, 4:7] = (v / np.sqrt((v * v).sum(-1, keepdims=True))).astype(F32)
    sets = {"coherent": torch.from_numpy(rays).cuda(), "permuted": torch.from_numpy(rays[perm]).cuda(),
            "random": torch.from_numpy(rnd).cuda()}
    times = {k: [] for k in ("features", *sets)}
    hits = {}
    for rep in range(a.reps + 1):  # round 0 warms up
        tr.set_seed(R.DEFAULT_SEED + 1 + rep)  # drops the cached feature buffer
        tr.features()
        f_ms = tr.denoise_times()["features_ms"]
        row = {"features": f_ms}
        for k, t in sets.items():
            out = tr.intersect(t)
            row[k] = tr.intersect_time()
            if rep == 0:
                hits[k] = round(float((out[:, 0] == 1).float().mean().item()), 4)
        if rep:
            for k, ms in row.items():
                times[k].append(ms)
    tr.close()
    s = {k: summary(ms) for k, ms in times.items()}
    spread = max((v["max_ms"] - v["min_ms"]) / v["median_ms"] for v in s.values())
    doc["scenes"][key] = {"scene": fname, "hit_fraction": hits, **s,
                          "coherent_over_features": round(s["features"]["median_ms"] / s["coherent"]["median_ms"], 3),
                          "permuted_over_coherent_time": round(s["permuted"]["median_ms"] / s["coherent"]["median_ms"], 3),
                          "largest_relative_spread": round(spread, 3)}
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print(json.dumps(doc))
