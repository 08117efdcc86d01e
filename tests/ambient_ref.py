"""Ambient occlusion's rule (include/rt2.h "Ambient occlusion", raytrace2_amd/csrc/ambient.h) in numpy float32, shared
by the host test and the GPU tests: the sample directions from oracle.unit_vectors, the ray records of a point batch
or of an image's feature records, and the counts from oracle.hit. numpy rounds every float32 operation on its own
and its float32 division and sqrt are correctly rounded, so the product must match word for word. Every array below
is float32; no Python float takes part in an operation."""
import functools

import numpy as np

import edge_rays as E
from helpers import SEED
from test_gpu_query import _valid

F32 = np.float32
FLT_MAX = np.finfo(F32).max
FRAME0 = 0x80000000  # the frame word of sample 0
INVALID = np.uint32(0xFFFFFFFF)
W, H, SAMPLES = 32, 18, 24  # the image the GPU test and the non-vacuity check share
# (scene, radius) of the image tests. Book 2's image is left out: its camera's first hits lie in the mist, every ray
# of a call meets the mist at one free-flight distance, so every count flips from 0 to `samples` between two radii
# and no radius gives a pixel with 0 < count < samples; book 2 runs in point mode. Perlin spheres at
# radius 0.5 gives 24 such pixels, too few, and runs at radius 2 only.
IMAGE_CASES = [("cornell_box_original", F32(100)), ("cornell_box_original", FLT_MAX),
               ("cornell_box_scene_graph", F32(100)), ("cornell_box_scene_graph", FLT_MAX),
               ("cornell_box_volume", F32(100)), ("cornell_box_volume", FLT_MAX),
               ("final_render_book_1", F32(2)), ("perlin_spheres", F32(2))]
BOOK2 = "book2_final_scene_10000_samples"


def near_zero(v):
    return (np.abs(v) <= F32(1e-8)).all(-1)


def directions(n, u):
    """d of the rule for normals n and unit-vector draws u, (..., 3) each."""
    n, u = np.asarray(n, F32), np.asarray(u, F32)
    v = n + u
    v = np.where(near_zero(v)[..., None], n, v)
    with np.errstate(all="ignore"):
        l2 = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
        return (v * (F32(1) / np.sqrt(l2))[..., None]).astype(F32)


@functools.lru_cache(maxsize=None)
def _draw(seed, i, s):
    from oracle.oracle import unit_vectors
    return unit_vectors(seed, int(i), FRAME0 + int(s), 1)[0]


def draws(seed, index, samples, first=0):
    """(len(index), samples, 3): the first RandUnitVec3 draw of the stream (seed, i, FRAME0 + s)."""
    return np.array([[_draw(seed, i, first + s) for s in range(samples)] for i in index], F32).reshape(len(index), samples, 3)


def sample_rays(points, index, samples, seed=SEED):
    """The ray records (n, samples, 8) of points (n, 8) with stream indices `index`, and which points are valid. The
    rays of an invalid point are not to be traced (zeros)."""
    points = np.asarray(points, F32).reshape(-1, 8)
    ok = _valid(points)
    rays = np.zeros((len(points), samples, 8), F32)
    if ok.any():
        u = draws(seed, np.asarray(index)[ok], samples)
        rays[ok, :, 0:4] = points[ok, None, 0:4]
        rays[ok, :, 4:7] = directions(points[ok, None, 4:7], u)
        rays[ok, :, 7] = points[ok, None, 7]
    return rays, ok


def image_points(features, radius, rows=None):
    """The point records (rows * W, 8) of features()-shaped records (rows, W, 16), their global pixel indices (rows:
    the global row of each local one, default all) and which pixels are hits."""
    f = np.asarray(features, F32)
    nrows, w = f.shape[0], f.shape[1]
    ys = np.arange(nrows) if rows is None else np.asarray(rows)
    pts = np.zeros((nrows, w, 8), F32)
    pts[..., 0:3] = f[..., 2:5]
    pts[..., 3] = F32(radius)
    pts[..., 4:7] = f[..., 5:8]
    index = (ys[:, None] * w + np.arange(w)[None, :]).reshape(-1)
    return pts.reshape(-1, 8), index, (f[..., 0] != 0).reshape(-1)


def image_rays(features, radius, samples, seed=SEED, rows=None):
    """(rays (n, samples, 8), traced (n,)): the rays of an image's pixels; traced: a hit pixel with a valid point."""
    pts, index, hit = image_points(features, radius, rows)
    pts[~hit] = 0  # (a miss: an invalid record)
    rays, ok = sample_rays(pts, index, samples, seed)
    return rays, ok & hit


def flags(scene_path, rays, seed=SEED):
    """oracle.hit's flag for rays (m, 8); a ray outside QueryRayValid is not traced and counts as clear."""
    rays = np.asarray(rays, F32).reshape(-1, 8)
    ok = _valid(rays)
    return np.array([int(E.hit(scene_path, r, seed)[0] == 1) if v else 0 for r, v in zip(rays, ok)], np.uint32)


def counts(scene_path, rays, traced, seed=SEED):
    """The counts (n,) uint32 of rays (n, samples, 8) from oracle.hit; INVALID where not traced."""
    n, k = rays.shape[0], rays.shape[1]
    out = np.full(n, INVALID, np.uint32)
    for i in np.flatnonzero(traced):
        out[i] = flags(scene_path, rays[i], seed).sum()
    assert k > 0
    return out


POINT_SAMPLES = 16
POINT_LIMIT = 300  # point records per scene
POINT_SCENES = ("cornell_box_original", "cornell_box_volume", "final_render_book_1", BOOK2)


@functools.lru_cache(maxsize=None)
def mist_distance(seed=SEED):
    """The free-flight distance at which every ray of a call meets book 2's mist (one medium stream per call): the
    largest t of 200 unbounded unit rays from inside the room, which all but a few reach."""
    g = np.random.default_rng(5)
    o = np.array([278, 278, -300], F32)
    ts = np.array([E.hit(E.scene_file(BOOK2), E.rays(o, E._unit(g.normal(size=3)).astype(F32))[0], seed)[1]
                   for _ in range(200)], F32)
    assert (ts > ts.max() * F32(0.999)).sum() >= 100  # (unit directions: the mist's t is one distance for all)
    return ts.max()


def point_radius(name):
    """Point mode's tmax per scene: book 2 below its mist's free-flight distance (half of it), book 1 at 2, the
    Cornell rooms at 100."""
    if name == BOOK2:
        return F32(mist_distance() * F32(0.5))
    return F32(2) if name == "final_render_book_1" else F32(100)


@functools.lru_cache(maxsize=None)
def edge_points(name):
    """Up to POINT_LIMIT point records from the hit rays of the scene's edge batch: the oracle's hit point (slots
    2-4) and normal (5-7), the ray's time, tmax = point_radius(name). Frozen."""
    b, a = E.batch(name), E.answers(name)
    hit = np.flatnonzero(a[:, 0] == 1)[:POINT_LIMIT]
    pts = np.zeros((len(hit), 8), F32)
    pts[:, 0:3] = a[hit, 2:5]
    pts[:, 3] = point_radius(name)
    pts[:, 4:7] = a[hit, 5:8]
    pts[:, 7] = b.rays[hit, 7]
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def oracle_points(name, seed=SEED, samples=POINT_SAMPLES):
    """(counts, rays, traced) of edge_points(name) by the oracle alone, frozen."""
    pts = edge_points(name)
    rays, traced = sample_rays(pts, np.arange(len(pts)), samples, seed)
    c = counts(E.scene_file(name), rays, traced, seed)
    for a in (c, rays, traced):
        a.setflags(write=False)
    return c, rays, traced


@functools.lru_cache(maxsize=None)
def oracle_features(name, seed=SEED, w=W, h=H):
    """features()-shaped records of the scene's own camera from oracle.hit, frozen."""
    from denoise_ref import features_ref
    from oracle.oracle import OracleScene
    o = OracleScene(E.scene_file(name), seed)
    f, _ = features_ref(o, o.camera_params(w, h, 16), w, h, seed)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def oracle_image(name, radius, seed=SEED, samples=SAMPLES):
    """(counts (H * W,), rays, traced) of the scene's image at W x H by the oracle alone, frozen."""
    rays, traced = image_rays(oracle_features(name, seed), radius, samples, seed)
    c = counts(E.scene_file(name), rays, traced, seed)
    for a in (c, rays, traced):
        a.setflags(write=False)
    return c, rays, traced
