"""Small scenes whose images the BVH's slab tests decide (DESIGN.md §4 "Flat walk of small BVHs"), authored
with raytrace2_amd.authoring.SceneDoc and written into a temporary directory.

Each scene is a corridor: the camera looks down -x, so the boxes lie in line along the BVH's longest axis, and
every box sits under a transform with scale >= 2. A transformed child reports model-space t (Transform.cpp:
13-20), so a hit on the far box, which the pre-order walk visits first, leaves a tmax of world distance / scale,
and the reference's world-space slab test then culls the subtree that holds the nearer box: the reference draws
the far box where a walk without slab tests draws the near one. The flat walk visits every leaf without a slab
test and must therefore leave exactly such lanes uncertified and trace the BVH program again for them; a kernel
that certified one of them would draw what the oracle draws under CTL_NO_SLAB.

  mix     A, B, C, D + FLOOR, BACK, LIGHT       7 leaves: mixed scales, one general-axis rotation
  eight   A, B, C, D, E' + FLOOR, BACK, LIGHT   8 leaves: the leaf limit (kFlatBvhMaxLeaves)
  nine    eight + F                             9 leaves: one past the limit, no flat program
  nonuni  A', B', C + FLOOR, BACK, LIGHT        6 leaves: non-uniform scales (8, 2, 4) and (16, 8, 8)
  norot   A, B unrotated + FLOOR, BACK, LIGHT   5 leaves: scale and translation only
  side    A, B, C, E' + FLOOR, LIGHT, SIDE      7 leaves: another wall set
  metal   A, B, C, E + FLOOR, LIGHT, SIDE       7 leaves: `side` with E of metal: specular bounces
  two     A, B                                  2 leaves: no inner node, so no slab test below the root: the control

E' is E with a diffuse material. The flat-walk kernel is an instantiation of the Cornell-box kernel alone
(render.hip kFlatVariant: transforms, no spheres, media, textures or specular materials), and the kernel variant
follows from the scene's material table (compile.cpp: any metal or dielectric entry sets kFeatSpecular). So a
scene that lists a metal is compiled with a flat program that no launch walks: `metal` is kept to pin exactly
that, and the material table of every other scene leaves the metal out (it is the last id, so the others keep
theirs).

`decided(name)` is the mask of the pixels whose oracle accumulation differs in any bit between the faithful
walk and CTL_NO_SLAB at the tests' render size, and D its count; a deciding scene must have D >= D_MIN (about
2 % of the image), so that a wrongly certified lane shows in the image. tests/test_flat_scenes_host.py checks
that on the CPU; tests/test_gpu_flat_scenes.py renders the scenes on the flat-walk kernel."""
import atexit
import functools
import os
import shutil
import tempfile

import numpy as np

from helpers import SEED

W, H, SPP, FRAMES = 70, 37, 16, 16  # 2,590 pixels: no multiple of 64
D_MIN = 50

# (world size, translation, rotation [deg, ax, ay, az] or None, scale, material)
BOXES = {
    "A": ((165, 165, 165), (0, 0, 0), (10, 0, 1, 0), (8, 8, 8), 0),
    "B": ((165, 165, 165), (600, 0, 0), (-10, 0, 1, 0), (16, 16, 16), 4),
    "C": ((80, 80, 80), (900, 0, 60), (25, 0.2, 1, 0.1), (32, 32, 32), 5),
    "D": ((60, 200, 60), (300, 0, 150), (40, 0, 1, 0), (8, 8, 8), 2),
    "E": ((50, 120, 50), (1000, 0, 120), (-35, 0, 1, 0), (4, 4, 4), 6),
    "F": ((40, 60, 40), (750, 0, -40), (5, 0, 1, 0), (2, 2, 2), 1),
}
BOXES["E_diffuse"] = BOXES["E"][:4] + (1,)
BOXES["A_nonuni"] = BOXES["A"][:3] + ((8, 2, 4),) + BOXES["A"][4:]
BOXES["B_nonuni"] = BOXES["B"][:3] + ((16, 8, 8),) + BOXES["B"][4:]
BOXES["A_norot"] = BOXES["A"][:2] + (None,) + BOXES["A"][3:]
BOXES["B_norot"] = BOXES["B"][:2] + (None,) + BOXES["B"][3:]
# (q, u, v, material)
QUADS = {
    "FLOOR": ((-100, 0, -200), (1300, 0, 0), (0, 0, 600), 1),
    "BACK": ((-50, 0, -200), (0, 400, 0), (0, 0, 600), 2),
    "LIGHT": ((300, 400, 0), (300, 0, 0), (0, 0, 200), 3),
    "SIDE": ((-100, 0, 400), (1300, 0, 0), (0, 400, 0), 0),
}
# scene -> boxes, then quads, in file order
SCENES = {
    "mix": ("A", "B", "C", "D", "FLOOR", "BACK", "LIGHT"),
    "eight": ("A", "B", "C", "D", "E_diffuse", "FLOOR", "BACK", "LIGHT"),
    "nine": ("A", "B", "C", "D", "E_diffuse", "F", "FLOOR", "BACK", "LIGHT"),
    "nonuni": ("A_nonuni", "B_nonuni", "C", "FLOOR", "BACK", "LIGHT"),
    "norot": ("A_norot", "B_norot", "FLOOR", "BACK", "LIGHT"),
    "side": ("A", "B", "C", "E_diffuse", "FLOOR", "LIGHT", "SIDE"),
    "metal": ("A", "B", "C", "E", "FLOOR", "LIGHT", "SIDE"),
    "two": ("A", "B"),
}
COMPILED_FLAT = ("mix", "eight", "nonuni", "norot", "side", "metal", "two")  # the compiler gives a flat program
FLAT = ("mix", "eight", "nonuni", "norot", "side", "two")  # ... and the flat-walk kernel walks it
DECIDING = ("mix", "eight", "nonuni", "norot", "side", "metal")  # the slab tests decide pixels (and `nine`'s)
METAL = 6
MATERIAL_A, MATERIAL_B = BOXES["A"][4], BOXES["B"][4]


def leaves(name):
    return len(SCENES[name])


def xforms(name):
    return sum(1 for n in SCENES[name] if n in BOXES)


def doc(name):
    from raytrace2_amd import authoring as A
    d = A.SceneDoc(fov=30, center=[1500, 120, 90], look_at=[0, 80, 80], width=600, aspect_ratio=1,
                   background=[0.3, 0.4, 0.6])
    d.lambertian([0.65, 0.05, 0.05])
    d.lambertian([0.73, 0.73, 0.73])
    d.lambertian([0.12, 0.45, 0.15])
    d.light([15, 15, 15])
    d.lambertian([0.1, 0.2, 0.8])
    d.lambertian([0.8, 0.7, 0.1])
    if any(n in BOXES and BOXES[n][4] == METAL for n in SCENES[name]):
        assert d.metal([0.8, 0.8, 0.8], 0.1) == METAL
    for n in SCENES[name]:
        if n in BOXES:
            size, t, rot, scale, m = BOXES[n]
            d.node(d.box([0, 0, 0], [s / k for s, k in zip(size, scale)], m), xform=A.transform(t, rot, scale))
        else:
            q, u, v, m = QUADS[n]
            d.node(d.quad(q, u, v, m))
    return d


@functools.lru_cache(maxsize=None)
def _dir():
    d = tempfile.mkdtemp(prefix="rt2_flat_scenes_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    for name in SCENES:
        doc(name).dump(os.path.join(d, name + ".json"))
    return d


def scene_file(name):
    return os.path.join(_dir(), name + ".json")


@functools.lru_cache(maxsize=None)
def oracle_render(name, mask=0, max_depth=50):
    """(accumulation, counters) of the oracle's forward render at the tests' size under control mask `mask`;
    computed once, read-only."""
    from oracle import oracle as O
    with O.controls(mask):
        acc, _, cnt = O.OracleScene(scene_file(name), SEED).render(W, H, SPP, FRAMES, max_depth=max_depth, forward=True)
    acc.setflags(write=False)
    return acc, cnt


@functools.lru_cache(maxsize=None)
def decided(name, max_depth=50):
    """(H, W) bool: the pixels whose accumulation the slab tests decide."""
    from oracle.oracle import CTL_NO_SLAB
    a, _ = oracle_render(name, 0, max_depth)
    b, _ = oracle_render(name, CTL_NO_SLAB, max_depth)
    m = (a.view(np.uint32) != b.view(np.uint32)).any(axis=2)
    m.setflags(write=False)
    return m


def four_leaf_rays(n=200, seed=5):
    """Rays of the four-leaf class (tests/cpp/flat_cert.cpp): from x = 1000 down -x through both A and B, with
    direction lengths 0.1 and 0.01. Returns (origins, directions), (n, 3) float32 each."""
    g = np.random.default_rng(seed)
    o = np.stack([np.full(n, 1000.0), g.uniform(5, 160, n), g.uniform(40, 120, n)], axis=1).astype(np.float32)
    s = np.where(np.arange(n) % 2, 0.1, 0.01)
    d = np.stack([-s, g.uniform(-1e-4, 1e-4, n) * s, g.uniform(-1e-4, 1e-4, n) * s], axis=1).astype(np.float32)
    return o, d
