#!/usr/bin/env python3
"""What the noise estimate costs on one GPU, on the headline workload (Cornell 1024^2 @ 1000 spp by default).

Two tracers of the same scene, one with moments on (rt2_tracer_enable_moments: the accumulate pass also
sums the samples' squares), render the workload in turn, `--reps` times each, in one session: Mray/s of
every step, and the median and spread of each side. Then the noise call's own time with moments on: HIP
events on the tracer's stream around rt2_tracer_noise (the noise kernel over all pixels + the read-back of
its per-workgroup partials), and the host's wall time of noise() and standard_error().
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import raytrace2_amd as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scene", default="cornell_box_original.json")
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--spp", type=int, default=1000)
ap.add_argument("--reps", type=int, default=4)
ap.add_argument("--noise-reps", type=int, default=10)
a = ap.parse_args()

sc = R.Scene(os.path.join(ROOT, "scenes", a.scene), R.DEFAULT_SEED)
stream = torch.cuda.Stream()


def make(moments):
    tr = R.RayTracer(sc, 0)
    tr.SetSamplesPerPixel(a.spp)
    tr.OnResize((a.size, a.size))
    if moments:
        tr.enable_moments()
        tr.set_stream(stream.cuda_stream)  # so that torch events can time the noise call
    return tr


def step(tr):
    tr.Reset()
    tr.synchronize()
    tr.reset_stats()
    t0 = time.perf_counter()
    tr.Render(a.spp)
    tr.synchronize()
    dt = time.perf_counter() - t0
    st = tr.stats()
    return {"ms": round(dt * 1e3, 2), "mray_s": round(st["rays"] / dt / 1e6, 1), "kernel_ms": round(st["kernel_ms"], 2)}


def summary(steps):
    v = [s["mray_s"] for s in steps]
    return {"median_mray_s": statistics.median(v), "min": min(v), "max": max(v),
            "spread_pct": round(100.0 * (max(v) - min(v)) / statistics.median(v), 2),
            "median_ms": statistics.median(s["ms"] for s in steps), "steps": steps}


off, on = make(False), make(True)
for tr in (off, on, off, on):  # warm-up: both launch slots' sample buffers, code objects
    step(tr)
runs = {"off": [], "on": []}
for _ in range(a.reps):  # alternated
    runs["off"].append(step(off))
    runs["on"].append(step(on))

ev_ms, wall_ms = [], []
for _ in range(a.noise_reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(stream)
    nz = on.noise(0.01)
    e1.record(stream)
    e1.synchronize()
    wall_ms.append((time.perf_counter() - t0) * 1e3)
    ev_ms.append(e0.elapsed_time(e1))
t0 = time.perf_counter()
on.standard_error()
sem_ms = (time.perf_counter() - t0) * 1e3

out = {"workload": f"{a.scene} {a.size}x{a.size} @ {a.spp} spp", "moments_off": summary(runs["off"]),
       "moments_on": summary(runs["on"]),
       "on_over_off": round(statistics.median(s["mray_s"] for s in runs["on"]) /
                            statistics.median(s["mray_s"] for s in runs["off"]), 4),
       "noise_call": {"device_event_ms_median": round(statistics.median(ev_ms), 4),
                      "device_event_ms_min": round(min(ev_ms), 4), "device_event_ms_max": round(max(ev_ms), 4),
                      "host_wall_ms_median": round(statistics.median(wall_ms), 4),
                      "standard_error_host_wall_ms": round(sem_ms, 3), "last": nz},
       "device_bytes_peak": {"off": off.stats()["device_bytes_peak"], "on": on.stats()["device_bytes_peak"]}}
print(json.dumps(out), flush=True)
off.close()
on.close()
