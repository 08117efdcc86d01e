#!/usr/bin/env python3
"""Generates tests/golden/ref/*.npy from the compiled reference (oracle/_ref/librt2_ref.so, built by
oracle/Makefile's ref target where the reference checkout is present). A fixture is data: what the reference's
own Hit and RayTracer::Update returned. tests/test_gpu_reference.py compares the kernels with them on the GPU;
tests/test_reference_build.py regenerates them from the live library and compares the bytes.

  <scene>_hits.npy    float32 (21 + 18*32*10,): the 21 camera words of ref_camera(32, 18, spp), then ref_hit's
                      10 floats (hit, t, point, normal, front_face, material) on the 32x18 pixel-centre rays
                      (time 0, t in (0.001, FLT_MAX)). One for every scene of test_gpu_parity.CASES without a
                      constant medium (a medium's hit takes log(), where the kernel's LogU may differ from
                      logf by an ulp).
  <scene>_depth1.npy  float32 (18, 32, 3): ref_render's accumulation at 32x18, spp setting 4, 6 frames,
                      max_depth 1, seed helpers.SEED. For scenes with no medium, no defocus and no noise
                      texture on an emitter the kernel's path stream and the reference's agree draw for draw
                      up to the first hit and the result is emission or background, so the kernel must equal
                      the reference's own Update.
  <scene>_edges.npy   float32 (n, 18), n <= 400: rays of the scene's edge batch (tests/edge_rays.py: every class,
                      pairs kept together), each as its 8 ray words followed by ref_hit's 10 floats on it
                      (t in (0.001, the ray's tmax), the ray's time); a miss has its record zeroed. One for every
                      scene without a medium and one for each node order of the authored scene `ties`.

Run from anywhere: python tests/golden/make_ref_golden.py"""
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(HERE, "ref")
SEED = 0x5EED2024  # helpers.SEED
W, H = 32, 18
DEPTH1_SPP, DEPTH1_FRAMES = 4, 6
# (scene, spp setting) of tests/test_gpu_parity.py::CASES
SCENES = [("cornell_box_original", 16), ("cornell_box_volume", 16), ("final_render_book_1", 500),
          ("book2_final_scene_10000_samples", 10000), ("checker_test", 64), ("perlin_spheres", 64),
          ("cornell_box_scene_graph", 16), ("cornell_box2", 16), ("light_scene1", 16)]
MAX_FILE, MAX_DIR = 64 * 1024, 512 * 1024


def scene_file(name):
    return os.path.join(ROOT, "scenes", name + ".json")


def _load(name):
    """(scene document, camera document): the camera may live in a file next to the scene."""
    doc = json.load(open(scene_file(name)))
    cam = doc.get("camera")
    if not isinstance(cam, dict):
        cam = json.load(open(os.path.join(ROOT, "scenes", (cam or "cam1") + ".json")))
    return doc, cam


def _primitives(doc):
    prims = doc["primitives"]
    return [p for group in prims.values() for p in group] if isinstance(prims, dict) else prims


def has_medium(name):
    return any("constant_medium" in p for p in _primitives(_load(name)[0]))


def _has_transform(nodes):
    return any("transform" in n or _has_transform(n.get("children", [])) for n in nodes)


def depth1_qualifies(name):
    doc, cam = _load(name)
    if has_medium(name) or cam.get("defocus_angle", 0.0) > 0:
        return False
    textures = doc.get("textures", [])
    return not any(m["type"] == "diffuse_light" and "tex_idx" in m and textures[m["tex_idx"]]["type"] == "noise"
                   for m in doc["materials"])


def hit_scenes():
    return [(n, spp) for n, spp in SCENES if not has_medium(n)]


def depth1_scenes():
    return [n for n, _ in SCENES if depth1_qualifies(n)]


def hit_fixture(name, spp):
    from denoise_ref import feature_rays
    from oracle.ref import RefScene
    r = RefScene(scene_file(name), SEED)
    cp = r.camera_params(W, H, spp)
    o, d = feature_rays(cp, W, H)
    rec = np.zeros((H, W, 10), np.float32)
    for y in range(H):
        for x in range(W):
            rec[y, x] = r.hit(o, d[y, x], seed=SEED)[:10]
    rec[rec[..., 0] == 0, 1:] = 0  # a miss leaves the record unspecified
    return np.concatenate([cp, rec.reshape(-1)]).astype(np.float32)


def depth1_fixture(name):
    from oracle.ref import RefScene
    acc, _ = RefScene(scene_file(name), SEED).render(W, H, DEPTH1_SPP, DEPTH1_FRAMES, max_depth=1, seed=SEED)
    return acc


def edge_scenes():
    import edge_rays as E
    return [n for n, _ in hit_scenes()] + list(E.TIES)


def edge_fixture(name):
    import edge_rays as E
    from oracle.ref import RefScene
    b, rows = E.batch(name), E.fixture_rows(name)
    r = RefScene(E.scene_file(name), SEED)
    out = np.zeros((len(rows), 18), np.float32)
    for k, i in enumerate(rows):
        ray = b.rays[i]
        rec = r.hit(ray[0:3], ray[4:7], float(ray[7]), 0.001, float(ray[3]), seed=SEED)[:10]
        out[k, :8] = ray
        if rec[0] == 1:
            out[k, 8:] = rec
    assert (out[:, 8] == 1).any() and (out[:, 8] == 0).any(), name
    return out


def fixtures():
    """{file name: array} of every fixture, from the live library."""
    out = {}
    for name in edge_scenes():
        out[name + "_edges.npy"] = edge_fixture(name)
    for name, spp in hit_scenes():
        out[name + "_hits.npy"] = hit_fixture(name, spp)
    d1 = depth1_scenes()
    assert len(d1) >= 4, d1
    assert any(any(c != 0 for c in _load(n)[0].get("background_color", [1, 1, 1])) for n in d1), "no lit background"
    assert any(_has_transform(_load(n)[0].get("scene", [])) for n in d1), "no transformed child"
    for name in d1:
        out[name + "_depth1.npy"] = depth1_fixture(name)
    for k, a in out.items():
        assert (a == 0).any() and (a != 0).any(), k
    return out


def encode(a):
    b = io.BytesIO()
    np.save(b, np.ascontiguousarray(a, np.float32), allow_pickle=False)
    return b.getvalue()


def main():
    os.makedirs(OUT, exist_ok=True)
    total = 0
    for k, a in fixtures().items():
        data = encode(a)
        assert len(data) <= MAX_FILE, (k, len(data))
        total += len(data)
        open(os.path.join(OUT, k), "wb").write(data)
        print("wrote", k, a.shape, len(data))
    assert total <= MAX_DIR, total
    print("total", total)


if __name__ == "__main__":
    sys.exit(main())
