"""Rays aimed at decision boundaries, built deterministically from the oracle and the scene files (numpy, fixed
seeds, oracle.hit; no GPU, no compiled reference). Random rays do not land within an ulp of an edge, a tie or a
tangent; these do, by construction:

  silhouette  300 pairs per scene: two directions from one origin whose outcome keys differ, bisected in float32
              until the midpoint equals an end bit for bit: the two rays differ by at most 1 ulp per component and
              the scene answers them differently.
  tmin        100 pairs per scene: a ray re-started at fl(P - s d) just in front of its own hit point P, s bisected
              in [0.0005, 0.002] to adjacent floats on "the surface is accepted" (a hit nearer than 0.003): it is
              from one origin and is passed from the other (the interval starts at 0.001).
  continue    200 rays per scene from recorded hit points, as a bounce starts: back along the ray, mirrored about
              the normal, and in the tangent plane with a normal component of +-2^-k |d|, k = 8..23, and with one
              component set to +0 and -0.
  tmax        150 pairs per scene: a hit ray again with tmax = t and with the float below t: the other end of the
              interval (quads accept t == tmax, spheres do not; below t nothing is left to hit).
  aimed       (the two Cornell rooms) rays from inside the room at the room's corners and edges, the light's, and
              the two blocks' world-space corners and edges, un-normalised and normalised.
  ties        an authored scene in two node orders (`ties`, `ties_swapped`): coplanar overlapping quads, a box
              standing on the floor seen from below, twin spheres, tangent rays, touching spheres, box edges and
              rays lying in a face's plane.

An outcome key is (flag, material, normal bits); a miss is (0,). Ray records have test_gpu_query._rays' layout
(ox oy oz tmax | dx dy dz time). Every batch is shuffled by a fixed permutation, its length is no multiple of 64 and
at most 2000."""
import atexit
import functools
import os
import shutil
import tempfile
from collections import namedtuple

import numpy as np

from bits import same_bits
from conftest import scene_path
from helpers import SEED

F32 = np.float32
FLT_MAX = np.finfo(F32).max
HALF = F32(0.5)
MEDIA = ("cornell_box_volume", "book2_final_scene_10000_samples")
AIMED = ("cornell_box_original", "cornell_box_volume")
TIES = ("ties", "ties_swapped")
TIE_CLASSES = ("quads", "below", "twins")
N_SILHOUETTE, N_TMIN, N_CONTINUE, N_TMAX = 300, 100, 200, 150
MAX_RAYS = 2000
NEAR_T = F32(0.003)  # a tmin pair's accepted surface lies nearer than this (s <= 0.002, plus a large sphere's root error)
FIXTURE_RAYS = 400
# where the random rays start: the box the scene's objects of interest fill (x0, y0, z0, x1, y1, z1)
BOXES = {"cornell_box_original": (0, 0, -200, 555, 555, 555), "cornell_box_volume": (0, 0, -200, 555, 555, 555),
         "cornell_box_scene_graph": (0, 0, -200, 555, 555, 555), "cornell_box2": (0, 0, -200, 555, 555, 555),
         "final_render_book_1": (-12, 0, -12, 12, 4, 12), "book2_final_scene_10000_samples": (-300, 0, -100, 600, 555, 600),
         "checker_test": (-6, -1, -6, 6, 5, 6), "perlin_spheres": (-8, -1, -8, 8, 9, 8), "light_scene1": (-8, -1, -8, 8, 9, 8)}
SCENES = list(BOXES)

# rays (n, 8) and, per ray: its class, the index of its pair partner or -1, and for the ties scene the material
# the tie rule expects in either node order or -1; stats counts draws, candidates and drops per paired class
Batch = namedtuple("Batch", "rays cls pair rule stats")


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def ulps(a, b):
    """Distance in units of the last place between float32 arrays (+0 and -0 are 0 apart)."""
    def order(x):
        i = np.ascontiguousarray(x, F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(order(a) - order(b))


def key(rec):
    """The outcome key of a 10-word (or longer) hit record."""
    if rec[0] != 1:
        return (0,)
    return (1, int(rec[9])) + tuple(int(w) for w in bits(rec[5:8]))


def keys(recs):
    return [key(r) for r in recs]


def rays(o, d, tmax=FLT_MAX, time=0.0):
    """(n, 8) float32 ray records: the layout of test_gpu_query._rays."""
    d = np.asarray(d, F32).reshape(-1, 3)
    r = np.zeros((len(d), 8), F32)
    r[:, 0:3] = np.asarray(o, F32)
    r[:, 3] = tmax
    r[:, 4:7] = d
    r[:, 7] = time
    return r


@functools.lru_cache(maxsize=None)
def oracle(path):
    from oracle.oracle import OracleScene
    return OracleScene(path, SEED)


def hit(path, ray, seed=SEED):
    return oracle(path).hit(ray[0:3], ray[4:7], time=float(ray[7]), tmin=0.001, tmax=float(ray[3]), seed=seed)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def _bisect(kf, a, b, ka, kb):
    """Float32 vectors a, b with kf(a) = ka != kb = kf(b): one end is replaced by fl(0.5 a + 0.5 b) until that
    midpoint equals an end bit for bit. Every component then differs by at most 1 ulp: a gap of 2 ulps has a float
    in its middle, and a step whose midpoint rounds to a in one component and to b in another closes a component."""
    for _ in range(600):
        m = HALF * a + HALF * b
        if same_bits(m, a) or same_bits(m, b):
            return a, b, ka, kb
        km = kf(m)
        if km == ka:
            a = m
        else:
            b, kb = m, km
    raise AssertionError("bisection did not end")


def _draw(g, name):
    """One random ray: origin uniform in the scene's box, unit direction, time in [0, 1)."""
    b = np.array(BOXES[name], np.float64)
    o = (b[:3] + g.random(3) * (b[3:] - b[:3])).astype(F32)
    d = _unit(g.normal(size=3)).astype(F32)
    t = min(F32(g.random()), np.nextafter(F32(1), F32(0)))
    return o, d, t


def _silhouette(name, path):
    g = np.random.default_rng(11)
    o_ = oracle(path)
    out, stats = [], dict(draws=0, candidates=0, dropped=0)
    while len(out) < 2 * N_SILHOUETTE and stats["draws"] < 40 * N_SILHOUETTE:
        stats["draws"] += 1
        o, d0, t = _draw(g, name)
        d1 = (d0 + F32(0.2) * _unit(g.normal(size=3)).astype(F32)).astype(F32)

        def kf(d):
            return key(o_.hit(o, d, time=float(t), seed=SEED))
        k0, k1 = kf(d0), kf(d1)
        if k0 == k1:
            continue
        stats["candidates"] += 1
        a, b, ka, kb = _bisect(kf, d0, d1, k0, k1)
        if ka == kb or ulps(a, b).max() > 1:
            stats["dropped"] += 1
            continue
        out += [rays(o, a, FLT_MAX, t)[0], rays(o, b, FLT_MAX, t)[0]]
    return np.array(out, F32).reshape(-1, 8), stats


def _tmin(name, path):
    g = np.random.default_rng(12)
    o_ = oracle(path)
    out, stats = [], dict(draws=0, candidates=0, dropped=0)
    while len(out) < 2 * N_TMIN and stats["draws"] < 40 * N_TMIN:
        stats["draws"] += 1
        o, d, t = _draw(g, name)
        rec = o_.hit(o, d, time=float(t), seed=SEED)
        if rec[0] != 1:
            continue
        p = rec[2:5].copy()

        def at(s):
            return (p - s * d).astype(F32)

        def near(x):  # the surface the ray started from, accepted
            r = o_.hit(x, d, time=float(t), seed=SEED)
            return bool(r[0] == 1 and r[1] < NEAR_T)
        lo, hi = F32(0.0005), F32(0.002)
        if near(at(lo)) or not near(at(hi)):
            continue
        stats["candidates"] += 1
        while True:
            m = HALF * lo + HALF * hi
            if m == lo or m == hi:
                break
            if near(at(m)):
                hi = m
            else:
                lo = m
        a, b = at(lo), at(hi)
        if ulps(a, b).max() > 1:  # adjacent s, but an origin component near 0 moved by 2 ulps: close it
            a, b, _, _ = _bisect(near, a, b, False, True)
        ka, kb = (key(o_.hit(x, d, time=float(t), seed=SEED)) for x in (a, b))
        if ka == kb or ulps(a, b).max() > 1:
            stats["dropped"] += 1
            continue
        out += [rays(a, d, FLT_MAX, t)[0], rays(b, d, FLT_MAX, t)[0]]
    return np.array(out, F32).reshape(-1, 8), stats


def _continue(name, path):
    g = np.random.default_rng(13)
    o_ = oracle(path)
    out, origin = [], 0
    while len(out) < N_CONTINUE:
        o, d, t = _draw(g, name)
        rec = o_.hit(o, d, time=float(t), seed=SEED)
        if rec[0] != 1:
            continue
        p, n = rec[2:5].copy(), rec[5:8].copy()
        dn = (d[0] * n[0] + d[1] * n[1]) + d[2] * n[2]
        tan = d.astype(np.float64) - float(dn) * n.astype(np.float64)
        if np.sqrt((tan * tan).sum()) < 1e-3:
            tan = np.cross(n.astype(np.float64), [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
        tan = _unit(tan).astype(F32)
        dirs = [-d, (d - F32(2) * dn * n).astype(F32)]
        for j in range(6):  # over a scene's 20 origins every k in 8..23 occurs with either sign
            i = origin * 6 + j
            s = F32(1.0 if (i // 16) % 2 == 0 else -1.0) * F32(2.0 ** -(8 + i % 16))
            dirs.append((tan + s * n).astype(F32))
        least = int(np.argmin(np.abs(tan)))
        for z in (F32(0.0), F32(-0.0)):
            v = tan.copy()
            v[least] = z
            dirs.append(v)
        out += [rays(p, v, FLT_MAX, t)[0] for v in dirs]
        origin += 1
    return np.array(out[:N_CONTINUE], F32)


def _tmax(name, path):
    g = np.random.default_rng(14)
    o_ = oracle(path)
    out = []
    while len(out) < 2 * N_TMAX:
        o, d, t = _draw(g, name)
        rec = o_.hit(o, d, time=float(t), seed=SEED)
        if rec[0] != 1 or rec[1] < F32(0.002):
            continue
        out += [rays(o, d, rec[1], t)[0], rays(o, d, np.nextafter(rec[1], F32(0)), t)[0]]
    return np.array(out, F32)


def _box_targets(lo, hi, per_edge):
    """The eight corners of a box and `per_edge` points on each of its twelve edges, in double."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c = np.array([[(lo, hi)[(i >> k) & 1][k] for k in range(3)] for i in range(8)])
    pts = list(c)
    for i in range(8):
        for k in range(3):
            if not (i >> k) & 1:
                a, b = c[i], c[i | (1 << k)]
                pts += [a + (b - a) * f for f in (np.arange(per_edge) + 0.37) / per_edge]
    return np.array(pts)


def _rot_y(pts, degrees, translation):
    """Points of a box under translate * rotate-about-y, in double (glm::angleAxis about (0, 1, 0))."""
    th = np.radians(degrees)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    w = np.stack([x * np.cos(th) + z * np.sin(th), y, -x * np.sin(th) + z * np.cos(th)], -1)
    return w + np.asarray(translation, np.float64)


def _aimed_rays(origins, targets, time=0.25):
    """Every origin at every target: fl(target - origin) as it is, and normalised in float32."""
    out = []
    tg = np.asarray(targets, np.float64).astype(F32)  # rounded once
    for o in np.asarray(origins, F32):
        d = tg - o
        ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        out += [rays(o, d, FLT_MAX, time), rays(o, d / ln[:, None], FLT_MAX, time)]
    return np.concatenate(out)


def _aimed():
    """The Cornell rooms: corners and edges of the room (0 and 555, exact floats), of the light, and of the two
    blocks in world space."""
    from raytrace2_amd.authoring import _BLOCKS
    room = _box_targets([0, 0, 0], [555, 555, 555], 3)
    q, u, v = np.array([113.0, 554, 127]), np.array([330.0, 0, 0]), np.array([0.0, 0, 305])
    lc = [q, q + u, q + u + v, q + v]
    light = list(lc)
    for i in range(4):
        light.append(lc[i] + (lc[(i + 1) % 4] - lc[i]) * 0.37)
    blocks = [_rot_y(_box_targets([0, 0, 0], far, 2), rot[0], tr) for tr, rot, far in _BLOCKS]
    origins = [[151.25, 420.5, 60.75], [430.125, 130.375, 110.875], [277.75, 300.25, 20.5]]
    return _aimed_rays(origins, np.concatenate([room, np.array(light)] + blocks))


# ---- the authored scene -------------------------------------------------------------------------------------------
FLOOR_Y = 0.0
QUADS = (((-8, 0, -8), 16.0), ((-4, 0, -4), 6.0), ((-1, 0, -1), 6.0))  # (corner, side): floor, Q1, Q2
TWIN_C, TOUCH_C, REST_C = (-6.0, 2.0, -6.0), (-6.0, 2.0, -4.0), (6.0, 1.0, 6.0)
BOX_A = ((5.5, 0.0, -7.0), (7.5, 2.5, -5.0))
BOX_R = ((0.0, 0.0, 0.0), (2.0, 3.0, 2.0), (-7.0, 0.0, 5.0), 30.0)  # a, b, translation, degrees about y
# children of the one list node, by name; the swapped order exchanges the tied primitives
ORDER = {"ties": ("floor", "q1", "q2", "s1", "s2", "s3", "s4", "box_a", "box_r"),
         "ties_swapped": ("box_a", "q2", "q1", "floor", "s2", "s1", "s3", "s4", "box_r")}
MATERIAL = {n: i for i, n in enumerate(ORDER["ties"])}  # one material per primitive: the record names the winner


def ties_doc(order):
    """Every primitive a child of one node, so that the reference's HittableList loop meets them in `order`: a
    quad accepts t == closest (Interval::Contains) and the later one wins, a sphere does not (Surrounds) and the
    earlier one wins."""
    from raytrace2_amd import authoring as A
    doc = A.SceneDoc(fov=40, center=[0, 6, -20], look_at=[0, 1, 0], width=64, background=[0.7, 0.8, 1.0])
    for i in range(len(MATERIAL)):
        doc.lambertian([0.1 + 0.1 * i, 0.5, 0.9 - 0.1 * i])
    prim = {}
    for n, (q, side) in zip(("floor", "q1", "q2"), QUADS):
        prim[n] = doc.quad(q, [side, 0, 0], [0, 0, side], MATERIAL[n])
    prim["s1"] = doc.sphere(TWIN_C, 1.0, MATERIAL["s1"])
    prim["s2"] = doc.sphere(TWIN_C, 1.0, MATERIAL["s2"])
    prim["s3"] = doc.sphere(TOUCH_C, 1.0, MATERIAL["s3"])  # touches the twins at (-6, 2, -5)
    prim["s4"] = doc.sphere(REST_C, 1.0, MATERIAL["s4"])  # rests on the floor at (6, 0, 6)
    prim["box_a"] = doc.box(BOX_A[0], BOX_A[1], MATERIAL["box_a"])
    prim["box_r"] = doc.box(BOX_R[0], BOX_R[1], MATERIAL["box_r"])
    children = []
    for n in order:
        c = {"primitive": prim[n]}
        if n == "box_r":
            c["transform"] = A.transform(BOX_R[2], [BOX_R[3], 0, 1, 0])
        children.append(c)
    doc.node(children=children)
    return doc


@functools.lru_cache(maxsize=None)
def _ties_dir():
    d = tempfile.mkdtemp(prefix="rt2_ties_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    for name in TIES:
        ties_doc(ORDER[name]).dump(os.path.join(d, name + ".json"))
    return d


def scene_file(name):
    """The scene's file: a shipped scene's, or the authored scene's in a temporary directory."""
    return os.path.join(_ties_dir(), name + ".json") if name in TIES else scene_path(name)


def _winner(cands, quad_rule):
    """(material expected in `ties`, in `ties_swapped`) among tied primitives: the later quad, the earlier sphere."""
    pick = max if quad_rule else min
    return tuple(MATERIAL[pick(cands, key=ORDER[o].index)] for o in TIES)


def _ties_parts():
    """{class: (rays, rule (n, 2))}. Origins are placed so that the tied surfaces are what a ray reaches first."""
    g = np.random.default_rng(21)
    none = (-1, -1)
    parts = {}
    # quads: from half a unit above, nearly straight down, onto the floor where 1, 2 or 3 coplanar quads overlap
    r, rule = [], []
    while len(r) < 200:
        x, z = g.uniform(-3.9, 4.5, 2)
        inside = ["floor"] + [n for n, (q, side) in zip(("q1", "q2"), QUADS[1:])
                              if q[0] + 0.05 < x < q[0] + side - 0.05 and q[2] + 0.05 < z < q[2] + side - 0.05]
        near_edge = any(min(abs(x - q[0]), abs(x - q[0] - s), abs(z - q[2]), abs(z - q[2] - s)) < 0.05 for q, s in QUADS[1:])
        if len(inside) < 2 or near_edge:
            continue
        o = np.array([x + g.uniform(-0.3, 0.3), g.uniform(0.3, 0.8), z + g.uniform(-0.3, 0.3)], F32)
        d = np.array([x, FLOOR_Y, z], F32) - o
        r.append(rays(o, d if len(r) % 2 else _unit(d), FLT_MAX, 0.25)[0])
        rule.append(_winner(inside, True))
    parts["quads"] = (np.array(r), np.array(rule))
    # below: from under the floor up into the untransformed box's footprint: the floor and the bottom face at one t
    r = []
    (ax, _, az), (bx, _, bz) = BOX_A
    for i in range(120):
        x, z = g.uniform(ax + 0.05, bx - 0.05), g.uniform(az + 0.05, bz - 0.05)
        o = np.array([x + g.uniform(-0.5, 0.5), -g.uniform(0.5, 2.0), z + g.uniform(-0.5, 0.5)], F32)
        d = np.array([x, FLOOR_Y, z], F32) - o
        r.append(rays(o, d if i % 2 else _unit(d), FLT_MAX, 0.25)[0])
    parts["below"] = (np.array(r), np.array([_winner(["floor", "box_a"], True)] * len(r)))
    # twins: from the side away from the touching sphere into the two identical spheres
    r = []
    c = np.array(TWIN_C)
    for i in range(200):
        v = _unit(g.normal(size=3))
        v[1], v[2] = abs(v[1]), -abs(v[2])
        o = (c + g.uniform(2.0, 5.0) * v).astype(F32)
        d = (c + 0.9 * g.uniform(-1, 1) * _unit(g.normal(size=3))).astype(F32) - o
        r.append(rays(o, d if i % 2 else _unit(d), FLT_MAX, 0.25)[0])
    parts["twins"] = (np.array(r), np.array([_winner(["s1", "s2"], False)] * len(r)))
    # tangent: through a point of a sphere, perpendicular to its radius
    r = []
    while len(r) < 120:
        c = np.array((TWIN_C, REST_C, TOUCH_C)[len(r) % 3])
        n = _unit(g.normal(size=3))
        n[1] = abs(n[1])
        d = _unit(np.cross(n, g.normal(size=3)))
        d = d if d[1] >= 0 else -d  # rising: past the sphere there is the background
        o = c + n - g.uniform(2.0, 4.0) * d
        if o[1] < 0.1:
            continue
        r.append(rays(o, d * (1.0 if len(r) % 2 else 3.25), FLT_MAX, 0.25)[0])
    parts["tangent"] = (np.array(r), np.array([none] * len(r)))
    # touch: at the point where two spheres touch, and at the point where a sphere rests on the floor
    r = []
    p = np.array([-6.0, 2.0, -5.0])
    for i in range(80):
        phi = g.uniform(-0.5, np.pi + 0.5)
        o = (p + g.uniform(2.0, 4.0) * np.array([np.cos(phi), np.sin(phi), g.uniform(-0.05, 0.05)])).astype(F32)
        d = p.astype(F32) - o
        r.append(rays(o, d if i % 2 else _unit(d), FLT_MAX, 0.25)[0])
    p = np.array([REST_C[0], FLOOR_Y, REST_C[2]])
    for i in range(60):
        phi, th = g.uniform(0, 2 * np.pi), g.uniform(0.0, 0.3) * (i % 3 != 0)  # every third lies in the floor's plane
        o = (p + g.uniform(2.0, 4.0) * np.array([np.cos(phi) * np.cos(th), np.sin(th), np.sin(phi) * np.cos(th)])).astype(F32)
        d = p.astype(F32) - o
        r.append(rays(o, d if i % 2 else _unit(d), FLT_MAX, 0.25)[0])
    parts["touch"] = (np.array(r), np.array([none] * len(r)))
    # box edges: both boxes' corners and edges from outside, from about the boxes' own height, so that a ray
    # which passes an upper edge goes on to the background
    r = []
    for tg, centre in ((_box_targets(BOX_A[0], BOX_A[1], 3), [6.5, 1.25, -6.0]),
                       (_rot_y(_box_targets(BOX_R[0], BOX_R[1], 3), BOX_R[3], BOX_R[2]),
                        _rot_y(np.array([[1.0, 1.5, 1.0]]), BOX_R[3], BOX_R[2])[0])):
        for t in tg:
            v = _unit(g.normal(size=3))
            v[1] = g.uniform(-0.2, 0.25)
            r.append(_aimed_rays([np.asarray(centre) + g.uniform(3.0, 5.0) * v], [t])[len(r) % 2])
    parts["box_edges"] = (np.array(r), np.array([none] * len(r)))
    # in a face's plane: direction components along the normal of exactly 0, of 1e-9 (|denominator| < 1e-8
    # rejects it though it is not parallel) and of 2e-8 (accepted); through the top and side planes of the
    # untransformed box, the rotated box's top, and along the floor
    r = []
    top = BOX_A[1][1]
    for i in range(100):
        ny = F32((0.0, -0.0, 1e-9, -1e-9, 2e-8, -2e-8)[i % 6])
        kind = (i // 6) % 4
        if kind == 0:    # in the top face's plane of the untransformed box, towards it
            o = np.array([g.uniform(2.0, 5.0), top, g.uniform(-7.5, -4.5)], F32)
            d = np.array([1.0, ny, g.uniform(-0.2, 0.2)], F32)
        elif kind == 1:  # in its side plane x = 5.5, from above and from the front
            o = np.array([BOX_A[0][0], g.uniform(0.5, 4.0), g.uniform(-10.0, -7.5)], F32)
            d = np.array([ny, g.uniform(-0.5, 0.2), 1.0], F32)
        elif kind == 2:  # along the floor, towards a box's foot or the resting sphere's point
            tg = (np.array([6.5, 0.0, -6.0]), np.array([REST_C[0], 0.0, REST_C[2]]), np.array([-6.0, 0.0, 5.5]))[(i // 24) % 3]
            # from a height of -T ny, so that the floor's own t is T > 0.001 wherever the denominator is accepted
            o = np.array([g.uniform(-3.0, 3.0), -g.uniform(0.5, 2.0) * float(ny), g.uniform(-3.0, 3.0)], F32)
            d = _unit(tg - o).astype(F32)
            d[1] = ny
        else:            # in the rotated box's top plane y = 3
            o = np.array([g.uniform(-3.5, -2.0), BOX_R[1][1], g.uniform(4.0, 7.0)], F32)
            d = np.array([-1.0, ny, g.uniform(-0.2, 0.2)], F32)
        r.append(rays(o, d, FLT_MAX, 0.25)[0])
    parts["inplane"] = (np.array(r), np.array([none] * len(r)))
    return parts


# ---- batches ------------------------------------------------------------------------------------------------------
def _assemble(parts, pairs, rules, stats):
    """Concatenates the classes, pads off a multiple of 64 with a copy of the first ray of the last class, and
    shuffles by a fixed permutation; pair partners are carried through it."""
    cls = np.concatenate([np.full(len(r), k) for k, r in parts.items()])
    allr = np.concatenate(list(parts.values())).astype(F32)
    pair = np.full(len(allr), -1, np.int64)
    rule = np.full((len(allr), 2), -1, np.int64)
    at = 0
    for k, r in parts.items():
        if k in pairs:
            i = at + np.arange(len(r))
            pair[i] = i ^ 1
            assert at % 2 == 0 and len(r) % 2 == 0
        if k in rules:
            rule[at:at + len(r)] = rules[k]
        at += len(r)
    if len(allr) % 64 == 0:
        allr, cls = np.concatenate([allr, allr[-1:]]), np.concatenate([cls, cls[-1:]])
        pair, rule = np.concatenate([pair, [-1]]), np.concatenate([rule, [[-1, -1]]])
    assert len(allr) % 64 != 0 and len(allr) <= MAX_RAYS
    perm = np.random.default_rng(2).permutation(len(allr))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    pair = np.where(pair[perm] >= 0, inv[np.maximum(pair[perm], 0)], -1)
    out = Batch(np.ascontiguousarray(allr[perm]), cls[perm], pair, rule[perm], stats)
    for a in (out.rays, out.cls, out.pair, out.rule):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def batch(name):
    """The scene's batch: one of SCENES, or "ties" (both node orders are asked the same rays). Built under the
    oracle's default controls."""
    from oracle import oracle as O
    assert O.lib().oracle_get_controls() == 0
    if name in TIES:
        tp = _ties_parts()
        parts = {k: v[0] for k, v in tp.items()}
        # the ties again at the interval's end: 40 rays of each tie class with tmax = t and the float below it
        # (all tied quads accept t == tmax, neither twin does)
        at = []
        for k in TIE_CLASSES:
            for r in parts[k][:40]:
                t = hit(scene_file("ties"), r)[1]
                at += [rays(r[0:3], r[4:7], t, r[7])[0], rays(r[0:3], r[4:7], np.nextafter(t, F32(0)), r[7])[0]]
        parts["tmax"] = np.array(at, F32)
        return _assemble(parts, ("tmax",), {k: v[1] for k, v in tp.items()}, {})
    path = scene_path(name)
    parts, stats = {}, {}
    parts["silhouette"], stats["silhouette"] = _silhouette(name, path)
    parts["tmin"], stats["tmin"] = _tmin(name, path)
    parts["continue"] = _continue(name, path)
    parts["tmax"] = _tmax(name, path)
    if name in AIMED:
        parts["aimed"] = _aimed()
    return _assemble(parts, ("silhouette", "tmin", "tmax"), {}, stats)


def nudged_keys_differ(name, r):
    """Whether moving one direction component of ray r by +-1 or +-4 ulps changes its outcome key."""
    k0 = key(hit(scene_file(name), r))
    for c in (4, 5, 6):
        for n in (1, -1, 4, -4):
            q = r.copy()
            for _ in range(abs(n)):
                q[c] = np.nextafter(q[c], F32(np.inf if n > 0 else -np.inf))
            if key(hit(scene_file(name), q)) != k0:
                return True
    return False


def fixture_rows(name):
    """At most FIXTURE_RAYS indices into batch(name): classes taken in turn, pairs kept together."""
    b = batch("ties" if name in TIES else name)
    units = {}
    for i in range(len(b.rays)):
        if b.pair[i] < 0:
            units.setdefault(str(b.cls[i]), []).append((i,))
        elif i < b.pair[i]:
            units.setdefault(str(b.cls[i]), []).append((i, int(b.pair[i])))
    rows = []
    while any(units.values()):
        for k in sorted(units):
            if units[k] and len(rows) + len(units[k][0]) <= FIXTURE_RAYS:
                rows += units[k].pop(0)
            else:
                units[k] = []
    return np.array(rows)


@functools.lru_cache(maxsize=None)
def answers(name):
    """oracle.hit's 10 words for every ray of the scene's batch, at SEED."""
    b = batch("ties" if name in TIES else name)
    a = np.array([hit(scene_file(name), r) for r in b.rays], F32)
    a.setflags(write=False)
    return a
