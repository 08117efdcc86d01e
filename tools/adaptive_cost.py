#!/usr/bin/env python3
"""What adaptive sampling buys and costs on one GPU, on the headline workload (Cornell 1024^2 @ 1000 spp)
and on book 1 (1920x1080 @ 500 spp) by default.

Per workload, in one session and alternated `--reps` times: a plain tracer's Render(spp) against an adaptive
tracer's render loop (threshold 0.02, window 1, at most spp frames, a check every N frames from frame N on
for each N of `--check-every`, 64 and 250 by default; the loop is rt2_tracer_render_adaptive's, unrolled here so that each step's launches
and each check can be timed). Reported: the sample fraction (sum of n_p over pixels x spp), the wall-time
ratio adaptive / uniform, the render kernels' ray rate (rays over the launches' own GPU time) of the steps
launched over an active list against the steps launched over every pixel of the same run — the coherence
cost of compaction — the fraction of the uniform render's rays and render-kernel time the adaptive one
needs (retired pixels tend to be the cheap ones, so rays fall less than samples), and the host's wall
time per check.
Writes one JSON line (one entry per workload and check interval) to --out (default
profiles/adaptive_cost.json) and prints it."""
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
ap.add_argument("--workloads", default="cornell_box_original.json:1024x1024:1000,final_render_book_1.json:1920x1080:500")
ap.add_argument("--threshold", type=float, default=0.02)
ap.add_argument("--window", type=int, default=1)
ap.add_argument("--check-every", default="64,250", help="check intervals in frames, each measured in turn")
ap.add_argument("--min-frames", type=int, default=0, help="first check at this frame (0: the check interval)")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_cost.json"))
a = ap.parse_args()


def make(sc, w, h, spp, adaptive):
    tr = R.RayTracer(sc, 0)
    tr.SetSamplesPerPixel(spp)
    tr.OnResize((w, h))
    if adaptive:
        tr.enable_moments()
        tr.enable_adaptive()
    return tr


def uniform(tr, spp):
    tr.Reset()
    tr.synchronize()
    tr.reset_stats()
    t0 = time.perf_counter()
    tr.Render(spp)
    tr.synchronize()
    dt = time.perf_counter() - t0
    st = tr.stats()
    return {"ms": dt * 1e3, "rays": st["rays"], "kernel_ms": st["kernel_ms"]}


def adaptive(tr, spp, npix, every, first):
    tr.Reset()
    tr.synchronize()
    tr.reset_stats()
    steps, checks_ms, out = [], [], None
    active, rays0, k0 = npix, 0, 0.0
    t0 = time.perf_counter()
    while tr.FrameIdx() < spp and active > 0:
        n = min(every, spp - tr.FrameIdx())
        tr.Render(n)
        tr.synchronize()
        st = tr.stats()
        steps.append({"frames": n, "active": active, "rays": st["rays"] - rays0, "kernel_ms": st["kernel_ms"] - k0})
        rays0, k0 = st["rays"], st["kernel_ms"]
        if tr.FrameIdx() >= max(first, 2):
            c0 = time.perf_counter()
            out = tr.adaptive_check(a.threshold, a.window)
            checks_ms.append((time.perf_counter() - c0) * 1e3)
            active = out["active"]
    dt = time.perf_counter() - t0
    return {"ms": dt * 1e3, "steps": steps, "checks_ms": checks_ms, "last": out}


def rate(steps):
    ms = sum(s["kernel_ms"] for s in steps)
    return round(sum(s["rays"] for s in steps) / ms / 1e3, 1) if ms > 0 else None  # Mray/s


results = []
for spec in a.workloads.split(","):
    scene, size, spp = spec.split(":")
    w, h = (int(v) for v in size.split("x"))
    spp, npix = int(spp), w * h
    sc = R.Scene(os.path.join(ROOT, "scenes", scene), R.DEFAULT_SEED)
    uni, ada = make(sc, w, h, spp, False), make(sc, w, h, spp, True)
    uniform(uni, spp)  # warm-up: sample buffers, code objects
    for every in (int(v) for v in a.check_every.split(",")):
        first = a.min_frames or every
        adaptive(ada, spp, npix, every, first)
        u_runs, a_runs = [], []
        for _ in range(a.reps):  # alternated
            u_runs.append(uniform(uni, spp))
            a_runs.append(adaptive(ada, spp, npix, every, first))
        last = a_runs[-1]
        full = [s for s in last["steps"] if s["active"] == npix]
        listed = [s for s in last["steps"] if s["active"] < npix]
        u_ms, a_ms = statistics.median(r["ms"] for r in u_runs), statistics.median(r["ms"] for r in a_runs)
        results.append({
            "workload": f"{scene} {w}x{h} @ {spp} spp",
            "rule": {"threshold": a.threshold, "window": a.window, "check_every": every, "min_frames": first},
            "frames": last["last"]["frames"] if last["last"] else spp,
            "sample_fraction": round(last["last"]["samples"] / (npix * spp), 4) if last["last"] else 1.0,
            "active_at_end": last["last"]["active"] if last["last"] else npix,
            "uniform_ms": [round(r["ms"], 1) for r in u_runs], "adaptive_ms": [round(r["ms"], 1) for r in a_runs],
            "wall_ratio_adaptive_over_uniform": round(a_ms / u_ms, 4),
            "ray_fraction": round(sum(s["rays"] for s in last["steps"]) / u_runs[-1]["rays"], 4),
            "kernel_ms_ratio": round(sum(s["kernel_ms"] for s in last["steps"]) / u_runs[-1]["kernel_ms"], 4),
            "uniform_kernel_mray_s": round(u_runs[-1]["rays"] / u_runs[-1]["kernel_ms"] / 1e3, 1),
            "full_launch_mray_s": rate(full), "list_launch_mray_s": rate(listed),
            "list_steps": len(listed), "full_steps": len(full),
            "active_per_step": [s["active"] for s in last["steps"]],
            "step_kernel_ms": [round(s["kernel_ms"], 2) for s in last["steps"]],
            "check_ms_median": round(statistics.median(last["checks_ms"]), 3) if last["checks_ms"] else None,
            "check_ms_max": round(max(last["checks_ms"]), 3) if last["checks_ms"] else None,
            "list_order": "tile-major (32x8 tiles of four 8x8 blocks)"})
    uni.close()
    ada.close()

line = json.dumps({"adaptive_cost": results})
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write(line + "\n")
print(line, flush=True)
