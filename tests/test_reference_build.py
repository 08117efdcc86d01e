"""The CPU restatement (oracle/rt_oracle.cpp) against the reference's own compiled src/cpu_raytrace
(oracle/_ref/librt2_ref.so, built by oracle/Makefile's ref target against the stand-ins under oracle/refshim),
bit for bit: the random streams, the camera, closest hits on thousands of rays per scene, whole paths through
the reference's RayTracer::Update, and the Perlin textures; then three checks that the comparison has teeth,
and that the committed fixtures of tests/golden/ref are what the live library gives.

Runs without a GPU. Where neither the library nor the reference checkout exists (a GPU machine) the file
skips; a checkout without the library is a failure of the build. Whole paths run at 24x18 in every scene (each
run takes well under a second)."""
import functools
import json
import os
import sys

import numpy as np
import pytest

import edge_rays as E
from bits import f32_bits, same_bits
from conftest import ROOT, scene_path
from denoise_ref import feature_rays
from helpers import SEED
from test_gpu_parity import CASES

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_ref_golden as G  # noqa: E402

from oracle import oracle as O  # noqa: E402
from oracle import ref as R  # noqa: E402

SCENES = [(c[0], c[3]) for c in CASES]
NAMES = [n for n, _ in SCENES]
SPP = dict(SCENES)
FLT_MAX = float(np.finfo(np.float32).max)
HIT_KEY = SEED
N_RANDOM = 2000


if not R.available() and not R.checkout_present():
    pytest.skip("no compiled reference and no reference checkout", allow_module_level=True)
# a checkout without the library is a build failure: every test below then fails on loading the library


def _pair(name, mask=O.CTL_REF_MATH):
    """The oracle's scene, loaded and used under `mask`, and the reference's."""
    with O.controls(mask):
        o = O.OracleScene(scene_path(name), SEED)
    return o, R.RefScene(scene_path(name), SEED)


# ---- streams ----------------------------------------------------------------------------------------------
KEYS = [(SEED, 0, 0), (SEED, 1, 0), (SEED, 431, 5), (0x0123456789ABCDEF, 24 * 18 - 1, 9999), (0, 0xFFFFFFFE, 0xFFFFFFFF),
        (SEED, 0xFFFFFFF0, 0)]  # the last one is the hit stream


@pytest.mark.parametrize("seed,pixel,frame", KEYS)
def test_streams(seed, pixel, frame):
    """The driver's Philox stream, read through the reference's RandReal() hook, is oracle.uniforms."""
    a, b = R.uniforms(seed, pixel, frame, 64), O.uniforms(seed, pixel, frame, 64)
    assert same_bits(a, b)
    assert len(np.unique(a)) > 60 and (a >= 0).all() and (a < 1).all()


# ---- camera -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_camera(name):
    o, r = _pair(name)
    for w, h in ((33, 18), (64, 64)):
        for spp in (4, SPP[name]):
            assert same_bits(r.camera_params(w, h, spp), o.camera_params(w, h, spp)), (w, h, spp)


def test_camera_moved_and_defocus():
    o, r = _pair("cornell_box_original")
    cam = ((250.5, 300.25, -650.0), (278.0, 250.0, 10.0), (0.1, 1.0, 0.0), 31.5, 0.0, 1.0)
    o.set_camera(*cam)
    r.set_camera(*cam)
    for w, h in ((33, 18), (64, 64)):
        for spp in (4, 16):
            a, b = r.camera_params(w, h, spp), o.camera_params(w, h, spp)
            assert same_bits(a, b) and a[9] == np.float32(250.5)
    o, r = _pair("final_render_book_1")
    a, b = r.camera_params(33, 18, 500), o.camera_params(33, 18, 500)
    assert same_bits(a, b) and a[18] > 0 and np.abs(a[12:18]).max() > 0  # a defocus disk


# ---- hits -------------------------------------------------------------------------------------------------
# where the random rays start: the box the scene's objects of interest fill (x0, y0, z0, x1, y1, z1)
BOXES = {"cornell_box_original": (0, 0, -200, 555, 555, 555), "cornell_box_volume": (0, 0, -200, 555, 555, 555),
         "cornell_box_scene_graph": (0, 0, -200, 555, 555, 555), "cornell_box2": (0, 0, -200, 555, 555, 555),
         "final_render_book_1": (-12, 0, -12, 12, 4, 12), "book2_final_scene_10000_samples": (-300, 0, -100, 600, 555, 600),
         "checker_test": (-6, -1, -6, 6, 5, 6), "perlin_spheres": (-8, -1, -8, 8, 9, 8), "light_scene1": (-8, -1, -8, 8, 9, 8)}
RAY_SEED = {n: 1 for n in NAMES}


def _kinds_by_material(name):
    """{material index: set of primitive kinds that use it} and the set of kinds the scene has, from the scene
    file. Kinds: quad (boxes are six quads), sphere, moving sphere, transformed child, medium."""
    doc = json.load(open(scene_path(name)))
    prims = doc["primitives"]
    by_mat, kinds = {}, set()

    def add(mat, kind):
        by_mat.setdefault(mat, set()).add(kind)
        kinds.add(kind)

    def base(p, group=None):
        if (group or p.get("type")) in ("quad", "quads", "box", "boxes"):
            return "quad"
        return "moving sphere" if any(p.get("displacement", [0, 0, 0])) else "sphere"

    if isinstance(prims, dict):
        for group, items in prims.items():
            for p in items:
                add(p.get("material_id", 0), base(p, group))
        return by_mat, kinds
    n_mat = len(doc["materials"])
    mat_of = []
    for p in prims:
        cm = p.get("constant_medium")
        if cm is not None:
            if "albedo" in cm:
                mat_of.append((n_mat, "medium"))
                n_mat += 1
            else:
                mat_of.append((cm["material"], "medium"))
        else:
            mat_of.append((p.get("material", 0), base(p)))

    def walk(node, transformed):
        transformed = transformed or "transform" in node
        if "primitive" in node:
            mat, kind = mat_of[node["primitive"]]
            add(mat, "transformed child" if transformed and kind != "medium" else kind)
            if transformed and kind == "medium":
                kinds.add("transformed child")
                by_mat.setdefault(mat, set()).add("transformed child")
        for c in node.get("children", []):
            walk(c, transformed)

    for node in doc["scene"]:
        walk(node, False)
    return by_mat, kinds


def _kinds_hit(name, recs):
    """The kinds that the hit records give evidence of: a material that only one kind uses; a medium's fixed
    normal (1, 0, 0) with front_face set on a medium's material; and, for a material that quads share with
    transformed quads, a normal off the axes (the scenes' untransformed quads are axis-aligned and their
    transforms rotate)."""
    by_mat, _ = _kinds_by_material(name)
    seen = set()
    for rec in recs:
        ks = by_mat.get(int(rec[9]), set())
        if len(ks) == 1:
            seen |= ks
        elif "medium" in ks:
            seen.add("medium")
            if "transformed child" in ks:
                seen.add("transformed child")
        elif ks == {"quad", "transformed child"}:
            seen.add("transformed child" if np.count_nonzero(np.abs(rec[5:8]) > 1e-3) >= 2 else "quad")
    return seen


@functools.lru_cache(maxsize=None)
def _rays(name):
    """(origins, directions, times) of the 32x18 pixel-centre rays followed by N_RANDOM random rays: origins
    uniform in the scene's box, unnormalised directions with lengths in [0.1, 10], time in [0, 1)."""
    o, _ = _pair(name)
    c, d = feature_rays(o.camera_params(32, 18, SPP[name]), 32, 18)
    d = d.reshape(-1, 3)
    g = np.random.default_rng(RAY_SEED[name])
    b = np.array(BOXES[name], np.float64)
    ro = b[:3] + g.random((N_RANDOM, 3)) * (b[3:] - b[:3])
    v = g.normal(size=(N_RANDOM, 3))
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * (0.1 * 100.0 ** g.random((N_RANDOM, 1)))
    t = g.random(N_RANDOM)
    origins = np.concatenate([np.repeat(c[None], len(d), 0), ro]).astype(np.float32)
    dirs = np.concatenate([d, v]).astype(np.float32)
    times = np.concatenate([np.zeros(len(d)), t]).astype(np.float32)
    ln = np.linalg.norm(dirs[len(d):].astype(np.float64), axis=1)
    assert ln.min() >= 0.0999 and ln.max() <= 10.001
    return origins, dirs, times


@pytest.mark.parametrize("name", NAMES)
def test_hits(name):
    """ref_hit against oracle.hit on the pixel-centre rays and 2000 random rays, a quarter of them with the
    interval ending or starting exactly at the first pass's t (Interval::Contains / Surrounds edges): the hit
    flag agrees on every ray and all 10 floats are bit-equal where hit. Media draw from the hit stream keyed by
    HIT_KEY + the ray's index on both sides (one key for all rays would give every ray the same free path)."""
    o, r = _pair(name)
    origins, dirs, times = _rays(name)
    n, first_random = len(origins), 32 * 18
    with O.controls(O.CTL_REF_MATH):
        tmin = np.full(n, 0.001, np.float32)
        tmax = np.full(n, FLT_MAX, np.float32)
        first = np.array([o.hit(origins[i], dirs[i], float(times[i]), seed=HIT_KEY + i) for i in range(n)])
        edge = first_random + np.arange(N_RANDOM // 4) * 4  # every fourth random ray
        for j, i in enumerate(edge):
            if first[i, 0] == 1:
                if j % 2 == 0:
                    tmax[i] = first[i, 1]
                else:
                    tmin[i] = first[i, 1]
        assert np.count_nonzero(first[edge, 0] == 1) >= 50  # the edges are exercised
        a = np.array([o.hit(origins[i], dirs[i], float(times[i]), float(tmin[i]), float(tmax[i]), seed=HIT_KEY + i)
                      for i in range(n)])
        b = np.array([r.hit(origins[i], dirs[i], float(times[i]), float(tmin[i]), float(tmax[i]), seed=HIT_KEY + i)
                      for i in range(n)])
    flags_differ = np.flatnonzero(a[:, 0] != b[:, 0])
    assert len(flags_differ) == 0, f"hit flag differs on rays {flags_differ[:5]}"
    hit = a[:, 0] == 1
    words = f32_bits(a[hit]) != f32_bits(b[hit][:, :10])
    assert not words.any(), f"{np.count_nonzero(words)} words differ, first ray {np.flatnonzero(hit)[np.argwhere(words)[0][0]]}"
    assert np.count_nonzero(hit) >= 200 and np.count_nonzero(~hit) >= 20, (np.count_nonzero(hit), np.count_nonzero(~hit))
    _, kinds = _kinds_by_material(name)
    seen = _kinds_hit(name, a[hit])
    assert seen >= kinds, f"no hit on {kinds - seen}"


# ---- hits at the decision boundaries ----------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES + list(E.TIES))
def test_edge_batches(name):
    """ref_hit against oracle.hit on the scene's edge batch (tests/edge_rays.py: pairs an ulp apart across a
    silhouette and across either end of the interval, rays leaving a surface, rays aimed at corners and edges;
    the authored scene's ties, tangents and in-plane rays in both node orders), the ray's own tmax and time: the
    flag agrees on every ray and all 10 floats are bit-equal where hit. Media are keyed by ray as in test_hits.
    Without a medium CTL_REF_MATH changes no hit, so these are also the answers the GPU tests compare with."""
    batch = E.batch(name)  # built under the default controls, as the GPU tests build it
    path = E.scene_file(name)
    with O.controls(O.CTL_REF_MATH):
        o = O.OracleScene(path, SEED)
        r = R.RefScene(path, SEED)
        args = [(q[0:3], q[4:7], float(q[7]), 0.001, float(q[3])) for q in batch.rays]
        a = np.array([o.hit(*x, seed=HIT_KEY + i) for i, x in enumerate(args)])
        b = np.array([r.hit(*x, seed=HIT_KEY + i) for i, x in enumerate(args)])
    flags_differ = np.flatnonzero(a[:, 0] != b[:, 0])
    assert len(flags_differ) == 0, f"hit flag differs on rays {flags_differ[:5]} ({batch.cls[flags_differ[:5]]})"
    hit = a[:, 0] == 1
    words = f32_bits(a[hit]) != f32_bits(b[hit][:, :10])
    assert not words.any(), f"{np.count_nonzero(words)} words differ, first ray {np.flatnonzero(hit)[np.argwhere(words)[0][0]]}"
    assert np.count_nonzero(hit) >= 0.1 * len(a) and np.count_nonzero(~hit) >= 0.1 * len(a)
    if name not in E.MEDIA:
        mine = E.answers(name)
        assert np.array_equal(mine[:, 0], a[:, 0]) and same_bits(mine[hit], a[hit])


# ---- whole paths ------------------------------------------------------------------------------------------
PW, PH = 24, 18


def _paths_differ(name, spp, frames, mask=O.CTL_REF_MATH, **kw):
    """Words that differ between the reference's Update and the oracle's recursive-order render, and the two
    counts of uniforms consumed."""
    o, r = _pair(name, mask)
    with O.controls(mask):
        oa, _, cnt = o.render(PW, PH, spp, frames, forward=False, threads=1, **kw)
    ra, draws = r.render(PW, PH, spp, frames, **kw)
    return int(np.count_nonzero(f32_bits(oa) != f32_bits(ra))), cnt["rng_draws"], draws, ra


@pytest.mark.parametrize("name", NAMES)
def test_whole_paths(name):
    """24x18, max_depth 50: spp setting 4 with 6 frames (the stratum indices wrap) and the scene's own setting
    with 3 frames. The reference is fed the oracle's uniforms, so every word is equal, NaNs included, and both
    consume the same number of uniforms."""
    for spp, frames in ((4, 6), (SPP[name], 3)):
        differ, o_draws, r_draws, acc = _paths_differ(name, spp, frames)
        assert differ == 0, f"{differ} of {acc.size} words differ at spp setting {spp}"
        assert o_draws == r_draws and r_draws > PW * PH * frames * 3
        assert (acc != 0).any()


@pytest.mark.parametrize("kw", [dict(max_depth=0), dict(max_depth=1), dict(max_depth=2), dict(frame_begin=5)],
                         ids=["depth0", "depth1", "depth2", "frame_begin5"])
def test_whole_paths_cornell_edges(kw):
    frames = 2 if "frame_begin" in kw else 6
    differ, o_draws, r_draws, acc = _paths_differ("cornell_box_original", 4, frames, **kw)
    assert differ == 0 and o_draws == r_draws
    if kw.get("max_depth") == 0:
        assert not acc.any() and r_draws == PW * PH * frames * 3  # the camera still draws


# ---- Perlin -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["perlin_spheres", "book2_final_scene_10000_samples"])
def test_perlin(name):
    """Noise::Value of every noise texture at 256 seeded points (half near the origin, half across the scene)
    against the oracle's texture value: the tables are drawn in the same order and the lattice sums round alike."""
    o, r = _pair(name)
    noise = [i for i, k in enumerate(r.info()[1]) if k == 2]
    assert noise and [i for i, t in enumerate(o.textures()) if int(t[0]) == 2] == noise
    g = np.random.default_rng(7)
    pts = np.concatenate([g.uniform(-10, 10, (128, 3)), g.uniform(-600, 600, (128, 3))]).astype(np.float32)
    for tex in noise:
        with O.controls(O.CTL_REF_MATH):
            a = o.texture_value(tex, pts)
        b = r.perlin_probe(tex, pts)
        assert same_bits(a, b), f"texture {tex}: {np.count_nonzero(f32_bits(a) != f32_bits(b))} words differ"
        assert len(np.unique(b)) > 200


# ---- power ------------------------------------------------------------------------------------------------
def test_power_world_t_is_seen():
    """Without the model-space-t quirk (Transform.cpp:13-20) the oracle no longer equals the reference."""
    assert _paths_differ("cornell_box_original", 4, 6, O.CTL_REF_MATH | O.CTL_WORLD_T)[0] > 0


def test_power_single_leaf_is_seen():
    """Without the doubly-tested span-1 BVH leaf (BVH.cpp:18-20, 50-55) book 2 differs."""
    assert _paths_differ("book2_final_scene_10000_samples", 4, 6, O.CTL_REF_MATH | O.CTL_SINGLE_LEAF)[0] > 0


def test_power_ref_math_is_needed():
    """With the restatement's own sampling maps (no CTL_REF_MATH) Cornell differs."""
    assert _paths_differ("cornell_box_original", 4, 6, 0)[0] > 0


# ---- fixtures ---------------------------------------------------------------------------------------------
def test_fixtures_are_what_the_library_gives():
    """Every file of tests/golden/ref holds exactly what the live library gives, and nothing else is there."""
    fresh = G.fixtures()
    assert sorted(os.listdir(G.OUT)) == sorted(fresh)
    total = 0
    for k, a in fresh.items():
        data = open(os.path.join(G.OUT, k), "rb").read()
        assert data == G.encode(a), k
        assert len(data) <= G.MAX_FILE
        total += len(data)
    assert total <= G.MAX_DIR
