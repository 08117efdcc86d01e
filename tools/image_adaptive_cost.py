#!/usr/bin/env python3
"""What adaptive sampling of the gathered image saves and costs, on one MI355X: a tracer over devices=[0] * 4 (four
partitions of interleaved 2-row bands on one GPU, device-local copies), at 1024^2, for the Cornell box and book 1:

  (a) the sample fraction: samples traced by image_render_adaptive(threshold, frames) over pixels * frames;
  (b) the wall time of that call (to the end of synchronize()) against Render(frames) on the same tracer with
      adaptive sampling switched off, `--reps` runs each after a first one, alternated;
  (c) what the stack of counts adds to a gather: rt2_stats.gather_ms (HIP events on the root's stream around the
      transfers and the root's kernel) of gather() with the counts and without;
  (d) per check, the largest part's active pixels over the parts' mean (image_part_adaptive): how evenly the
      interleaved bands keep the remaining work spread.

The four partitions share one GPU: the run contains no xGMI traffic, and the parts' launches share the GPU's CUs, so
(b) is not the time of four GPUs. Writes one JSON line to --out (default profiles/image_adaptive_cost.json) and
prints it."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401

import raytrace2_amd as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scenes", default="cornell_box_original.json,final_render_book_1.json")
ap.add_argument("--size", default="1024x1024")
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--step", type=int, default=16, help="frames between checks")
ap.add_argument("--threshold", type=float, default=0.05)
ap.add_argument("--window", type=int, default=1)
ap.add_argument("--parts", type=int, default=4)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_adaptive_cost.json"))
a = ap.parse_args()
w, h = (int(v) for v in a.size.split("x"))
npix = w * h


def summary(xs, digits=3):
    rest = xs[1:]
    return {"first": round(xs[0], digits), "median": round(statistics.median(rest), digits), "min": round(min(rest), digits),
            "max": round(max(rest), digits), "runs": len(rest)}


def timed(tr, call):
    tr.Reset()
    tr.synchronize()
    t0 = time.perf_counter()
    out = call()
    tr.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def gather_ms(tr):
    g0 = tr.stats()["gather_ms"]
    tr.gather()
    tr.synchronize()
    return tr.stats()["gather_ms"] - g0


def measure(scene):
    sc = R.Scene(os.path.join(ROOT, "scenes", scene), R.DEFAULT_SEED)
    tr = R.RayTracer(sc, devices=[0] * a.parts)
    tr.SetSamplesPerPixel(a.frames)
    tr.OnResize((w, h))
    tr.enable_moments()
    wall = {"image_render_adaptive_ms": [], "render_ms": []}
    gathers = {"with_counts_ms": [], "without_counts_ms": []}
    last = None
    for _ in range(a.reps + 1):  # alternated
        tr.image_enable_adaptive(True)
        ms, last = timed(tr, lambda: tr.image_render_adaptive(a.threshold, a.frames, window=a.window, check_every=a.step))
        wall["image_render_adaptive_ms"].append(ms)
        gathers["with_counts_ms"].append(gather_ms(tr))
        tr.image_enable_adaptive(False)
        ms, _ = timed(tr, lambda: tr.Render(a.frames))
        wall["render_ms"].append(ms)
        gathers["without_counts_ms"].append(gather_ms(tr))
    # (d) the loop by hand, to read every check's parts
    tr.image_enable_adaptive(True)
    checks = []
    while tr.FrameIdx() < a.frames:
        tr.Render(min(a.step, a.frames - tr.FrameIdx()))
        out = tr.image_adaptive_check(a.threshold, a.window)
        active = [tr.image_part_adaptive(p)["active"] for p in range(a.parts)]
        mean = sum(active) / len(active)
        checks.append({"frames": out["frames"], "active": out["active"], "retired": out["retired"], "parts_active": active,
                       "largest_over_mean": round(max(active) / mean, 4) if mean else None})
        if out["active"] == 0:
            break
    tr.close()
    res = {"frames": last["frames"], "active": last["active"], "samples": last["samples"],
           "sample_fraction": round(last["samples"] / (npix * a.frames), 4),
           "wall": {k: summary(v) for k, v in wall.items()}, "gather_gpu": {k: summary(v, 4) for k, v in gathers.items()},
           "checks": checks}
    res["adaptive_over_render_wall"] = round(res["wall"]["image_render_adaptive_ms"]["median"] / res["wall"]["render_ms"]["median"], 3)
    res["counts_add_to_gather_ms"] = round(res["gather_gpu"]["with_counts_ms"]["median"] -
                                           res["gather_gpu"]["without_counts_ms"]["median"], 4)
    return res


line = json.dumps({"image_adaptive_cost": {
    "workload": f"{w}x{h}, up to {a.frames} frames (samples_per_pixel {a.frames}), checks every {a.step} frames, threshold "
                f"{a.threshold}, window {a.window}; devices=[0] * {a.parts}, 2-row bands",
    "physical_gpus": 1, "not_measured": "more than one physical GPU: no xGMI traffic, no third ncclGather, no all-reduce "
                                        "over a communicator larger than 1; the parts share one GPU's CUs",
    "scenes": {s: measure(s) for s in a.scenes.split(",")}}})
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write(line + "\n")
print(line, flush=True)
