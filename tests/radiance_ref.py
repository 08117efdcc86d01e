"""The camera's own rays in numpy (include/rt2.h "Radiance queries"): Camera::GetRay restated in
float32 from oracle.camera_params, oracle.uniforms and oracle.cos_sin_2pi, every operation rounded on its own, with the
stream words and the number of draws GetRay took, so that RayTracer.radiance on these rays has a bit-exact statement:
the oracle's render of the same frames. The cases of tests/test_gpu_radiance.py and their oracle renders, shared (no
GPU)."""
import functools

import numpy as np

from conftest import scene_path
from helpers import SEED

F32 = np.float32
FLT_MAX = np.finfo(F32).max
SPP = 100           # the spp setting (strata: 10 x 10)
FRAME0, FRAMES = 3, 16
FRAME_WORD0 = 0x40000000  # radiance.h kRadianceFrame0
INVALID = np.uint32(0xFFFFFFFF)

# (scene, w, h, first_draw, non-zero pixels of the 16 frames, distinct per-pixel ray counts, pixels that change at
# max_depth 5 (None: not a max_depth case)): measured on the oracle, asserted in tests/test_radiance_host.py
CASES = [
    ("cornell_box_original", 16, 16, 3, 95, 134, 62),
    ("cornell_box_scene_graph", 16, 16, 3, 159, 115, 84),
    ("cornell_box_volume", 16, 16, 3, 205, 108, 104),
    ("final_render_book_1", 24, 14, 5, 336, 78, 144),
    ("book2_final_scene_10000_samples", 16, 16, 3, 99, 136, 17),
    ("perlin_spheres", 16, 12, 3, 192, 46, 35),
    ("light_scene1", 16, 12, 3, 58, 28, None),
    ("checker_test", 16, 12, 5, 192, 72, 108),
]
CASE = {c[0]: c for c in CASES}
NAMES = [c[0] for c in CASES]
DEPTH5 = [c[0] for c in CASES if c[6] is not None]
MIN_INFORMATIVE = 50


@functools.lru_cache(maxsize=None)
def oracle(name, seed=SEED):
    from oracle.oracle import OracleScene
    return OracleScene(scene_path(name), seed)


def _v(p, k):
    return p[3 * k:3 * k + 3].astype(F32)


def camera_rays(name, w, h, frames, seed=SEED, spp=SPP):
    """GetRay for every pixel of every frame in `frames`: rays (len(frames), h * w, 8) float32, streams (.., 2) uint32
    = (y * w + x, f), and first_draw, the uniforms GetRay took from the stream (3, or 5 with defocus)."""
    from oracle import oracle as O
    p = oracle(name).camera_params(w, h, spp)
    p00, du, dv, center, dfu, dfv = (_v(p, k) for k in range(6))
    defocus = not (p[18] <= 0)
    rs, sq = F32(p[19]), int(p[20])
    first_draw = 5 if defocus else 3
    frames = list(frames)
    rays = np.zeros((len(frames), h * w, 8), F32)
    streams = np.zeros((len(frames), h * w, 2), np.uint32)
    for k, f in enumerate(frames):
        s_i, s_j = F32(f % sq), F32(f // sq % sq)
        for y in range(h):
            for x in range(w):
                i = y * w + x
                u = O.uniforms(seed, i, f, 5)
                px = F32(F32(s_i + u[0]) * rs) - F32(0.5)
                py = F32(F32(s_j + u[1]) * rs) - F32(0.5)
                pc = (p00 + F32(F32(x) + px) * du) + F32(F32(y) + py) * dv
                c, time = center, u[2]
                if defocus:
                    r = np.sqrt(u[2], dtype=F32)
                    cd, sd = O.cos_sin_2pi(np.array([u[3]], F32))[0]
                    c = (center + F32(r * cd) * dfu) + F32(r * sd) * dfv
                    time = u[4]
                v = (pc - c).astype(F32)
                l2 = F32(F32(v[0] * v[0]) + F32(v[1] * v[1])) + F32(v[2] * v[2])
                d = v * (F32(1) / np.sqrt(l2, dtype=F32))
                rays[k, i, 0:3], rays[k, i, 3], rays[k, i, 4:7], rays[k, i, 7] = c, FLT_MAX, d, time
                streams[k, i] = (i, f)
    assert rays.dtype == F32
    return rays, streams, first_draw


@functools.lru_cache(maxsize=None)
def case_rays(name, seed=SEED):
    """The case's rays of frames FRAME0 .. FRAME0 + FRAMES - 1, read-only (shared among the tests)."""
    _, w, h, first_draw = CASE[name][:4]
    rays, streams, fd = camera_rays(name, w, h, range(FRAME0, FRAME0 + FRAMES), seed)
    assert fd == first_draw
    rays.setflags(write=False)
    streams.setflags(write=False)
    return rays, streams, fd


@functools.lru_cache(maxsize=None)
def case_render(name, max_depth=50, seed=SEED):
    """oracle.render of the case's frames in the forward product order: (accum (h, w, 3), ray_counts (h, w)), read-only."""
    _, w, h = CASE[name][:3]
    acc, rc, _ = oracle(name).render(w, h, SPP, FRAMES, frame_begin=FRAME0, max_depth=max_depth, seed=seed, forward=True)
    acc.setflags(write=False)
    rc.setflags(write=False)
    return acc, rc


def frame_sum(samples):
    """(frames, n, 3) float32 -> (n, 3): ((0 + s_0) + s_1) + ... in float32, oracle_render's accumulation."""
    acc = np.zeros(samples.shape[1:], F32)
    for s in np.asarray(samples, F32):
        acc = (acc + s).astype(F32)
    return acc


def depth1_from_hits(name, rays):
    """The depth-1 radiance of rays (n, 8) from oracle.hit on (0.001, tmax): the light's emission (its texture's value
    at the hit), the background on a miss, 0 otherwise. Media-free scenes, or rays whose media draws do not matter."""
    o = oracle(name)
    mats = o.materials()
    bg = np.array(list(o.info().background), F32)
    out = np.zeros((len(rays), 3), F32)
    for i, r in enumerate(rays):
        rec = o.hit(r[0:3], r[4:7], time=float(r[7]), tmin=0.001, tmax=float(r[3]), seed=SEED)
        if rec[0] == 0:
            out[i] = bg
        else:
            m = mats[int(rec[9])]
            if int(m[0]) == LIGHT_TYPE:
                out[i] = o.texture_value(int(m[6]), rec[2:5])[0]
    return out


LIGHT_TYPE = 4  # rt2_layout.h kMatDiffuseLight (checked against the library in tests/test_radiance_host.py)
