"""Rays aimed at the boundaries of the occlusion answer, built deterministically from the oracle and the scene files
(numpy, fixed seeds, oracle.hit; no GPU, no compiled reference). tests/edge_rays.py's pairs decide *which* surface
wins; few of them differ in the flag alone (17 pairs on book 1). These do, by construction:

  shadow  120 pairs per scene: two directions from one origin under one finite tmax = fl((0.05 + 0.95 u) * the
          diagonal of the scene's box) whose oracle flags differ, bisected in float32 by the flag alone until every
          component differs by at most 1 ulp: one ray of the pair is occluded within tmax, its neighbour is not.
  tmax3   100 hit rays per scene with t >= 0.002, three times each: tmax = the float below t, t, and the float
          above t. Below t nothing is left to hit, above t the hit is inside; at t a quad accepts (Contains) and a
          sphere does not (Surrounds).

The answer wanted is the flag of oracle.hit(o, d, time, 0.001, tmax) at SEED. Ray records have edge_rays.rays'
layout. A batch is shuffled by a fixed permutation and its length is no multiple of 64."""
import functools
from collections import namedtuple

import numpy as np

import edge_rays as E
from edge_rays import BOXES, SEED, _bisect, _draw, oracle, rays, scene_file, ulps  # noqa: F401

F32 = np.float32
N_SHADOW, N_TMAX3 = 120, 100
DRAW_LIMIT = 6000
# the authored ties scene has no entry in edge_rays.BOXES: the box its primitives fill
TIES_BOX = (-8, 0, -8, 8, 4, 8)
ALL = E.SCENES + list(E.TIES)

# rays (n, 8); per ray its class, the index of its pair partner (shadow) or -1, its place in its triple (tmax3:
# 0, 1, 2) or -1, and the oracle's flag at SEED; stats counts draws, candidates and drops of the shadow pairs
Batch = namedtuple("Batch", "rays cls pair slot flag stats")


def _box(name):
    return np.array(BOXES[name] if name in BOXES else TIES_BOX, np.float64)


def _draw_in(g, name):
    """edge_rays._draw, also for the authored scene (the same draws from the generator)."""
    if name in BOXES:
        return _draw(g, name)
    b = _box(name)
    o = (b[:3] + g.random(3) * (b[3:] - b[:3])).astype(F32)
    d = E._unit(g.normal(size=3)).astype(F32)
    t = min(F32(g.random()), np.nextafter(F32(1), F32(0)))
    return o, d, t


def flag(path, ray, seed=SEED):
    """The occlusion answer of a valid ray: oracle.hit's flag on (0.001, tmax)."""
    return int(E.hit(path, ray, seed)[0])


def _shadow(name, path):
    g = np.random.default_rng(21)
    o_ = oracle(path)
    b = _box(name)
    diag = float(np.sqrt(((b[3:] - b[:3]) ** 2).sum()))
    out, stats = [], dict(draws=0, candidates=0, dropped=0)
    while len(out) < 2 * N_SHADOW and stats["draws"] < DRAW_LIMIT:
        stats["draws"] += 1
        o, d0, t = _draw_in(g, name)
        d1 = (d0 + F32(0.2) * E._unit(g.normal(size=3)).astype(F32)).astype(F32)
        tmax = F32((0.05 + 0.95 * g.random()) * diag)

        def kf(d):
            return int(o_.hit(o, d, time=float(t), tmin=0.001, tmax=float(tmax), seed=SEED)[0])
        k0, k1 = kf(d0), kf(d1)
        if k0 == k1:
            continue
        stats["candidates"] += 1
        a, c, ka, kc = _bisect(kf, d0, d1, k0, k1)
        if ka == kc or ulps(a, c).max() > 1:
            stats["dropped"] += 1
            continue
        out += [rays(o, a, tmax, t)[0], rays(o, c, tmax, t)[0]]
    return np.array(out, F32).reshape(-1, 8), stats


def _tmax3(name, path):
    g = np.random.default_rng(22)
    o_ = oracle(path)
    out = []
    while len(out) < 3 * N_TMAX3:
        o, d, t = _draw_in(g, name)
        rec = o_.hit(o, d, time=float(t), seed=SEED)
        if rec[0] != 1 or rec[1] < F32(0.002):
            continue
        for tm in (np.nextafter(rec[1], F32(0)), rec[1], np.nextafter(rec[1], F32(np.inf))):
            out.append(rays(o, d, tm, t)[0])
    return np.array(out, F32)


@functools.lru_cache(maxsize=None)
def batch(name):
    """The scene's flag batch: one of edge_rays.SCENES or TIES. Built under the oracle's default controls."""
    from oracle import oracle as O
    assert O.lib().oracle_get_controls() == 0
    path = scene_file(name)
    sh, stats = _shadow(name, path)
    t3 = _tmax3(name, path)
    allr = np.concatenate([sh, t3]).astype(F32)
    cls = np.concatenate([np.full(len(sh), "shadow"), np.full(len(t3), "tmax3")])
    pair = np.full(len(allr), -1, np.int64)
    pair[:len(sh)] = np.arange(len(sh)) ^ 1
    slot = np.full(len(allr), -1, np.int64)
    slot[len(sh):] = np.arange(len(t3)) % 3
    if len(allr) % 64 == 0:
        allr, cls = np.concatenate([allr, allr[-1:]]), np.concatenate([cls, ["pad"]])
        pair, slot = np.concatenate([pair, [-1]]), np.concatenate([slot, [-1]])
    perm = np.random.default_rng(2).permutation(len(allr))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    pair = np.where(pair[perm] >= 0, inv[np.maximum(pair[perm], 0)], -1)
    r = np.ascontiguousarray(allr[perm])
    fl = np.array([flag(path, x) for x in r], np.int8)
    out = Batch(r, cls[perm], pair, slot[perm], fl, stats)
    for a in (out.rays, out.cls, out.pair, out.slot, out.flag):
        a.setflags(write=False)
    return out


def triples(b):
    """(m, 3) indices into the batch: each tmax3 ray's three records, in the order below t, t, above t. The three
    records of one ray share origin, direction and time, and no two tmax3 rays do."""
    idx = np.flatnonzero(b.cls == "tmax3")
    groups = {}
    for i in idx:
        groups.setdefault(b.rays[i, [0, 1, 2, 4, 5, 6, 7]].tobytes(), [None] * 3)[int(b.slot[i])] = int(i)
    return np.array(list(groups.values()), np.int64)
