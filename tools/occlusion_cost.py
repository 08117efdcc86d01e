#!/usr/bin/env python3
"""What an occlusion query costs next to a closest-hit query on one GPU (rt2.h "Ray queries"):
Cornell and book 1, 1024^2 rays per call.

Five batches of rays per scene, each once through RayTracer.occluded and once through RayTracer.intersect in every
round, both by the device entry on the same CUDA tensor (no copies in the time), alternated, timed with the
library's own HIP events around the kernel (rt2_tracer_intersect_time):
  - coherent:    the un-normalised pixel-centre rays pc - center of the scene's camera, in image order, tmax FLT_MAX;
  - permuted:    the same rays in one fixed random permutation;
  - random:      unit directions from random points in the scene's box, tmax FLT_MAX;
  - random_half: the random rays with tmax = 2 u t (t: the ray's own closest hit, u uniform in [0, 1)), so that
                 about half of the rays that hit something end in mid-air before it;
  - shadow:      from the first-hit points of the pixel-centre rays towards the scene's light (Cornell: the centre of
                 its light quad; book 1: a fixed point above the scene), d = light - point, tmax 0.999; a pixel
                 that hit nothing sends its ray from the camera.
One warm-up round, then `--reps` alternated rounds; medians, with min and max as the run-to-run spread, and per
batch the ratio intersect / occluded of the medians with the range the spreads allow.
Writes one JSON document to --out (default profiles/occlusion_cost.json) and prints it."""
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

# (scene file, the box random origins are drawn from: lo, hi, the point shadow rays aim at)
SCENES = {"cornell": ("cornell_box_original.json", (0.0, 0.0, 0.0), (555.0, 555.0, 555.0), (278.0, 554.0, 279.5)),
          "book1": ("final_render_book_1.json", (-11.0, 0.0, -11.0), (11.0, 3.0, 11.0), (0.0, 20.0, 0.0))}

ap = argparse.ArgumentParser()
ap.add_argument("--size", default="1024x1024")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occlusion_cost.json"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("occlusion_cost: needs a GPU")
w, h = (int(v) for v in a.size.split("x"))
n = w * h
F32 = np.float32
FLT_MAX = np.finfo(F32).max


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "mray_s": round(n / statistics.median(ms) / 1e3, 1), "calls": len(ms)}


doc = {"rays_per_call": n, "size": [w, h], "reps": a.reps, "version": R.lib.rt2_version().decode(), "scenes": {}}
for key, (fname, lo, hi, light) in SCENES.items():
    sc = R.Scene(os.path.join(ROOT, "scenes", fname), R.DEFAULT_SEED)
    tr = R.RayTracer(sc, 0)
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
    # the bounded and the shadow rays come from the closest hits of the unbounded ones (set-up, not timed)
    rec = tr.intersect(rnd)
    half = rnd.copy()
    hit = rec[:, 0] == 1
    half[hit, 3] = np.maximum(F32(2.0) * rng.random(n).astype(F32)[hit] * rec[hit, 1], F32(0.002))
    rec = tr.intersect(rays)
    hit = rec[:, 0] == 1
    shadow = np.zeros((n, 8), F32)
    shadow[:, 0:3] = np.where(hit[:, None], rec[:, 2:5], np.asarray(c, F32))
    shadow[:, 3] = F32(0.999)
    shadow[:, 4:7] = np.asarray(light, F32) - shadow[:, 0:3]
    sets = {"coherent": rays, "permuted": rays[perm], "random": rnd, "random_half": half, "shadow": shadow}
    sets = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in sets.items()}
    times = {k: {"occluded": [], "intersect": []} for k in sets}
    frac = {}
    for rep in range(a.reps + 1):  # round 0 warms up
        for k, t in sets.items():
            occ = tr.occluded(t)
            o_ms = tr.intersect_time()
            out = tr.intersect(t)
            i_ms = tr.intersect_time()
            if rep == 0:
                if not torch.equal(occ, out[:, 0].to(torch.int8)):
                    sys.exit(f"occlusion_cost: {key} {k}: occluded differs from intersect's flag")
                frac[k] = {"occluded": round(float((occ == 1).float().mean().item()), 4),
                           "not_traced": round(float((occ < 0).float().mean().item()), 4)}
            else:
                times[k]["occluded"].append(o_ms)
                times[k]["intersect"].append(i_ms)
    tr.close()
    res = {}
    for k, t in times.items():
        o, i = summary(t["occluded"]), summary(t["intersect"])
        res[k] = {**frac[k], "occluded_kernel": o, "intersect_kernel": i,
                  "intersect_over_occluded": round(i["median_ms"] / o["median_ms"], 3),
                  "ratio_min": round(i["min_ms"] / o["max_ms"], 3), "ratio_max": round(i["max_ms"] / o["min_ms"], 3),
                  "relative_spread": round(max((o["max_ms"] - o["min_ms"]) / o["median_ms"],
                                               (i["max_ms"] - i["min_ms"]) / i["median_ms"]), 3)}
    doc["scenes"][key] = {"scene": fname, "light": list(light), "batches": res}
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print(json.dumps(doc))
