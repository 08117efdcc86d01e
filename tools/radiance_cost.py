#!/usr/bin/env python3
"""What a radiance query costs on one GPU next to the render of the same frames (rt2.h "Radiance queries", DESIGN.md
§6m): Cornell and book 1 at 1024^2.

Per scene, the camera's rays of 1 frame and of 16 frames (frame-major, rows within a frame) are built on the device in
torch by Camera::GetRay's expression with torch's generator for the jitter, the lens and the time (the same distribution
of rays as the render's, not the same bits: the path streams are the render's, (pixel, frame) with first_draw 3 or 5, so
the paths after the first segment draw what the render draws) and sent through the device entry
(rt2_tracer_radiance_device) with counts, timed by the library's own HIP events around its kernels
(rt2_tracer_radiance_time). Per round, alternated: the query with refill, the query with RT2_RADIANCE_REFILL=0, and the
tracer's own render of the same number of frames from a reset (rt2_stats.kernel_ms and rays). One warm-up round, then
`--reps` rounds; medians with min and max as the run-to-run spread, rays per second both ways. Then one probe-shaped
call: 4,096 rays (one image row's worth, taken across the image) x 4,096 samples, with and without refill.
Writes one JSON document to --out (default profiles/radiance_cost.json) and prints it."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import raytrace2_amd as R  # noqa: E402
from raytrace2_amd._native import RadianceParams, check, lib  # noqa: E402

SCENES = {"cornell": "cornell_box_original.json", "book1": "final_render_book_1.json"}

ap = argparse.ArgumentParser()
ap.add_argument("--size", default="1024x1024")
ap.add_argument("--frames", default="1,16")
ap.add_argument("--probe", default="4096x4096", help="rays x samples of the probe-shaped call")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radiance_cost.json"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("radiance_cost: needs a GPU")
w, h = (int(v) for v in a.size.split("x"))
FLT_MAX = float(np.finfo(np.float32).max)


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "calls": len(v)}


def camera_rays(sc, frames, gen):
    """(frames * h * w, 8) float32 rays and (.., 2) int32 stream words on the device, and first_draw."""
    p = sc.camera_params(w, h, a.spp)
    dev = torch.device("cuda")
    v3 = [torch.tensor(p[3 * k:3 * k + 3], device=dev) for k in range(6)]
    p00, du, dv, center, dfu, dfv = v3
    defocus = not (p[18] <= 0)
    rs, sq = float(p[19]), int(p[20])
    f = torch.arange(frames, device=dev).view(-1, 1, 1)
    y = torch.arange(h, device=dev, dtype=torch.float32).view(1, -1, 1)
    x = torch.arange(w, device=dev, dtype=torch.float32).view(1, 1, -1)
    u = torch.rand((5, frames, h, w), device=dev, generator=gen)
    px = ((f % sq).float() + u[0]) * rs - 0.5
    py = ((f // sq % sq).float() + u[1]) * rs - 0.5
    pc = p00 + (x + px)[..., None] * du + (y + py)[..., None] * dv
    c = center.expand_as(pc)
    if defocus:
        r, phi = torch.sqrt(u[2]), 2 * np.pi * u[3]
        c = center + (r * torch.cos(phi))[..., None] * dfu + (r * torch.sin(phi))[..., None] * dfv
    d = torch.nn.functional.normalize(pc - c, dim=-1)
    rays = torch.empty((frames, h, w, 8), device=dev)
    rays[..., 0:3], rays[..., 3], rays[..., 4:7], rays[..., 7] = c, FLT_MAX, d, u[4]
    pix = (torch.arange(h, device=dev).view(1, -1, 1) * w + torch.arange(w, device=dev).view(1, 1, -1)).expand(frames, h, w)
    st = torch.stack([pix, f.expand(frames, h, w)], -1).to(torch.int32)
    return rays.view(-1, 8).contiguous(), st.view(-1, 2).contiguous(), 5 if defocus else 3


def query(tr, rays, st, prm, out, cnt, refill):
    """One device-entry call; its kernels' ms by the library's events."""
    if refill:
        os.environ.pop("RT2_RADIANCE_REFILL", None)
    else:
        os.environ["RT2_RADIANCE_REFILL"] = "0"
    torch.cuda.synchronize()
    check(lib.rt2_tracer_radiance_device(tr._h, rays.shape[0], ctypes.c_void_p(rays.data_ptr()),
                                         ctypes.c_void_p(st.data_ptr()) if st is not None else None, ctypes.byref(prm),
                                         R.DEFAULT_SEED, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(cnt.data_ptr())))
    tr.synchronize()
    os.environ.pop("RT2_RADIANCE_REFILL", None)
    return tr.radiance_time()


def rates(t, rays_cast):
    return {**summary(t), "grays_s": round(rays_cast / statistics.median(t) / 1e6, 2)}


doc = {"size": [w, h], "reps": a.reps, "spp_setting": a.spp, "version": lib.rt2_version().decode(), "scenes": {}}
for key, fname in SCENES.items():
    sc = R.Scene(os.path.join(ROOT, "scenes", fname), R.DEFAULT_SEED)
    tr = R.RayTracer(sc, 0)
    tr.SetSamplesPerPixel(a.spp)
    tr.OnResize((w, h))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    entry = {"scene": fname, "frames": {}}
    for frames in (int(v) for v in a.frames.split(",")):
        rays, st, fd = camera_rays(sc, frames, gen)
        n = rays.shape[0]
        out = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        cnt = torch.empty((n,), dtype=torch.int32, device="cuda")
        prm = RadianceParams(1, 0, fd)
        t = {"refill": [], "no_refill": [], "render": []}
        cast = render_rays = 0
        for rep in range(a.reps + 1):  # round 0 warms up
            on = query(tr, rays, st, prm, out, cnt, True)
            if rep == 0:
                cast = int(cnt.to(torch.int64).sum().item())
                first = out.clone()
            off = query(tr, rays, st, prm, out, cnt, False)
            if rep == 0 and not torch.equal(out.view(torch.int32), first.view(torch.int32)):
                sys.exit(f"radiance_cost: {key}: the answers differ without refill")
            tr.Reset()
            tr.synchronize()
            s0 = tr.stats()
            tr.Render(frames)
            tr.flush()
            tr.synchronize()
            s1 = tr.stats()
            if rep:
                t["refill"].append(on)
                t["no_refill"].append(off)
                t["render"].append(s1["kernel_ms"] - s0["kernel_ms"])
                render_rays = s1["rays"] - s0["rays"]
        r_on, r_off, r_render = rates(t["refill"], cast), rates(t["no_refill"], cast), rates(t["render"], render_rays)
        entry["frames"][str(frames)] = {
            "rays": n, "first_draw": fd, "rays_cast": cast, "render_rays_cast": render_rays, "refill": r_on,
            "no_refill": r_off, "render": r_render,
            "refill_gain": round(r_off["median_ms"] / r_on["median_ms"], 3),
            "refill_gain_min": round(r_off["min_ms"] / r_on["max_ms"], 3),
            "refill_gain_max": round(r_off["max_ms"] / r_on["min_ms"], 3),
            "query_over_render_per_ray": round((r_on["median_ms"] / cast) / (r_render["median_ms"] / render_rays), 3)}
        del rays, st, out, cnt
    # the probe-shaped call: few rays, many samples
    pn, pk = (int(v) for v in a.probe.split("x"))
    rays, st, fd = camera_rays(sc, 1, gen)
    pick = torch.linspace(0, rays.shape[0] - 1, pn, device="cuda").long()
    rays, st = rays[pick].contiguous(), st[pick].contiguous()
    out = torch.empty((pn, 3), dtype=torch.float32, device="cuda")
    cnt = torch.empty((pn,), dtype=torch.int32, device="cuda")
    prm = RadianceParams(pk, 0, fd)
    t = {"refill": [], "no_refill": []}
    for rep in range(a.reps + 1):
        on = query(tr, rays, st, prm, out, cnt, True)
        cast = int(cnt.to(torch.int64).sum().item())
        off = query(tr, rays, st, prm, out, cnt, False)
        if rep:
            t["refill"].append(on)
            t["no_refill"].append(off)
    entry["probe"] = {"rays": pn, "samples": pk, "rays_cast": cast, "refill": rates(t["refill"], cast),
                      "no_refill": rates(t["no_refill"], cast)}
    tr.close()
    doc["scenes"][key] = entry
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print(json.dumps(doc))
