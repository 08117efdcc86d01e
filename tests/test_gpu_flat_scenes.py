"""Scenes whose images the slab tests decide, on the flat-walk kernel (render.hip render_kernel<... | kFeatFlat>;
DESIGN.md §4 "Flat walk of small BVHs"). The committed Cornell-type scenes leave 34 of 1.9 million rays
uncertified, and their images do not change when the BVH's nodes never reject: a flat kernel that certified every
lane would pass every bit-identity test on them. The scenes of tests/flat_scenes.py are built so that it cannot:
in D of the 2,590 pixels (95 to 254, tests/test_flat_scenes_host.py) a path casts a ray on which the walk with
the slab tests and the walk without them disagree, so that a wave holds lanes that keep their flat hit beside
lanes the second trace rewrites. They also bring what no committed scene has: scaled transforms, uniform or not,
a rotation about a general axis (the matrix path beside kXformYAxis), up to five transforms, up to 43 steps, a
BVH at the 8-leaf limit and one past it.

Every render is 70 x 37 at spp 16, 16 frames. The oracle's renders and the mask of the D decided pixels are
computed once (flat_scenes.oracle_render, decided) and left unchanged.

The lower bound D <= flat_uncertified is derived, not measured: up to a pixel's first diverging ray its path is
the same under both oracles; on that ray the two walks disagree, so the certificate must leave it open; distinct
pixels give distinct rays.

The number of hits under RT2_FLAT_BVH=2 is, as in test_gpu_flat_bvh.py, the flat kernel's own count of the hits
its falling-back wave-bounces end with, bounded from outside by rays - paths <= hits <= rays.

`metal` is not among the flat scenes. The flat-walk kernel exists for the Cornell-box variant alone (transforms,
nothing else), and a material table that lists a metal selects a variant with specular materials: the scene is compiled
with a flat program (flat_steps 35) that no launch walks. The test pins that: the oracle's bits from the BVH
walk, no flat counter moves. `side` is the same scene with that box diffuse, on the flat kernel."""
import numpy as np
import pytest

import flat_scenes as S
import raytrace2_amd as R
from helpers import SEED
from raytrace2_amd.tracer import local_rows

pytestmark = pytest.mark.gpu

COUNTERS = ("flat_uncertified", "flat_wave_fallbacks", "flat_fallback_hits")
MODES = (None, "0", "2")  # RT2_FLAT_BVH at scene load: the flat program, none, a kernel that certifies no hit
PATHS = S.W * S.H * S.FRAMES


def render(name, *, max_depth=50, stats=False, launch_frames=0, partition=None):
    sc = R.Scene(S.scene_file(name), SEED)
    tr = R.RayTracer(sc, 0)
    tr.set_seed(SEED)
    tr.SetSamplesPerPixel(S.SPP)
    tr.max_depth = max_depth
    if stats:
        tr.enable_stats(True)
    tr.OnResize((S.W, S.H))
    if partition is not None:
        tr.set_partition(*partition)
    if launch_frames:
        tr.set_launch_frames(launch_frames)
    tr.Render(S.FRAMES)
    acc = tr.Accumulation().copy()
    st = tr.stats()
    variant = tr.last_launch()["variant"]
    tr.close()
    return sc.info(), acc, st, variant


def render_modes(monkeypatch, name, **kw):
    out = {}
    for mode in MODES:
        if mode is None:
            monkeypatch.delenv("RT2_FLAT_BVH", raising=False)
        else:
            monkeypatch.setenv("RT2_FLAT_BVH", mode)
        out[mode] = render(name, **kw)
    monkeypatch.delenv("RT2_FLAT_BVH", raising=False)
    return out


def brief(st):
    return {k: st[k] for k in ("rays", "paths") + COUNTERS}


def assert_oracle_bits(what, acc, o_acc, mask):
    """Bit identity; a failure names the first differing pixels and says which of them the slab tests decide."""
    assert acc.shape == o_acc.shape, (what, acc.shape, o_acc.shape)
    bad = (acc.view(np.uint32) != o_acc.view(np.uint32)).any(axis=2)
    if not bad.any():
        return
    ys, xs = np.nonzero(bad)
    n_dec = int((bad & mask).sum())
    first = ", ".join(f"({x}, {y}) {'decided' if mask[y, x] else 'ordinary'} got {acc[y, x].tolist()} want {o_acc[y, x].tolist()}"
                      for y, x in list(zip(ys, xs))[:6])
    verdict = []
    if n_dec:
        verdict.append(f"certified a decided lane ({n_dec} of the {int(mask.sum())} slab-decided pixels differ)")
    if n_dec < bad.sum():
        verdict.append(f"broke an ordinary lane ({int(bad.sum()) - n_dec} pixels no slab test decides differ)")
    raise AssertionError(f"{what}: {int(bad.sum())} pixels differ from the oracle: {' and '.join(verdict)}; first: {first}")


def check_flat_scene(name, runs, max_depth=50):
    """The assertions on one scene's three renders (the flat program, none, certifying nothing)."""
    o_acc, o_cnt = S.oracle_render(name, 0, max_depth)
    mask = S.decided(name, max_depth)
    d = int(mask.sum())
    (info, acc, st, variant), (info0, acc0, st0, variant0), (info2, acc2, st2, variant2) = (runs[m] for m in MODES)
    print(f"{name} max_depth {max_depth}: D {d}, oracle rays {o_cnt['rays']}, flat_steps {info.flat_steps} of "
          f"{info.linear_steps}, variants {variant} {variant0} {variant2}; default {brief(st)}; RT2_FLAT_BVH=0 {brief(st0)}; "
          f"RT2_FLAT_BVH=2 {brief(st2)}")
    assert_oracle_bits(f"{name}: the flat walk", acc, o_acc, mask)
    assert_oracle_bits(f"{name}: RT2_FLAT_BVH=0", acc0, o_acc, mask)
    assert_oracle_bits(f"{name}: RT2_FLAT_BVH=2 (every hit traced again)", acc2, o_acc, mask)
    assert st["rays"] == st0["rays"] == st2["rays"] == o_cnt["rays"]
    assert st["paths"] == st0["paths"] == st2["paths"] == PATHS
    # the flat kernel really ran
    assert info.flat_steps == info2.flat_steps > 0 and info0.flat_steps == 0
    assert info.flat_steps < info.linear_steps == info0.linear_steps
    assert st0["flat_uncertified"] == st0["flat_wave_fallbacks"] == st0["flat_fallback_hits"] == 0
    assert st2["flat_uncertified"] == st2["flat_fallback_hits"]
    assert st2["rays"] - st2["paths"] <= st2["flat_uncertified"] <= st2["rays"], brief(st2)
    assert (st2["flat_uncertified"] + 63) // 64 <= st2["flat_wave_fallbacks"] <= st2["flat_uncertified"]
    if name in S.DECIDING:  # the mixed regime: some lanes keep their flat hit, others are rewritten
        assert d >= S.D_MIN
        assert d <= st["flat_uncertified"] < st2["flat_uncertified"], (d, brief(st), brief(st2))
        assert 0 < st["flat_wave_fallbacks"] <= st["flat_uncertified"], brief(st)
    else:
        assert d == 0 and st["flat_uncertified"] <= st2["flat_uncertified"]
    return st, st2


@pytest.mark.parametrize("name", [n for n in S.FLAT if n in S.DECIDING])
def test_slab_decided_scenes_change_no_bit(have_gpu, monkeypatch, name):
    check_flat_scene(name, render_modes(monkeypatch, name))


def test_slab_decided_lanes_beside_lanes_that_sit_out(have_gpu, monkeypatch):
    """`eight` at max_depth 2: a path that ended waits for the wave's longest, so lanes sit out traces their
    neighbours run. The uncertified lanes are a function of the rays alone: two runs count the same."""
    st, st2 = check_flat_scene("eight", render_modes(monkeypatch, "eight", max_depth=2), max_depth=2)
    again = render_modes(monkeypatch, "eight", max_depth=2)
    assert again[None][2]["flat_uncertified"] == st["flat_uncertified"]
    assert again["2"][2]["flat_uncertified"] == st2["flat_uncertified"]
    o_acc, _ = S.oracle_render("eight", 0, 2)
    assert_oracle_bits("eight at max_depth 2, second run", again[None][1], o_acc, S.decided("eight", 2))


def test_one_leaf_past_the_limit_keeps_its_bvh_walk(have_gpu, monkeypatch):
    """`nine` is `eight` and one small box: kFlatBvhMaxLeaves from the other side."""
    o_acc, o_cnt = S.oracle_render("nine")
    for mode, (info, acc, st, variant) in render_modes(monkeypatch, "nine").items():
        print("nine", mode, "variant", variant, brief(st))
        assert info.flat_steps == 0 and info.n_top_nodes == 9
        assert st["flat_uncertified"] == st["flat_wave_fallbacks"] == st["flat_fallback_hits"] == 0
        assert st["rays"] == o_cnt["rays"]
        assert_oracle_bits(f"nine, RT2_FLAT_BVH={mode}", acc, o_acc, S.decided("nine"))


def test_a_listed_metal_keeps_the_bvh_walk(have_gpu, monkeypatch):
    """`metal`: compiled with a flat program, rendered by a kernel with specular materials, which walks the BVH program
    (see the module's docstring). Were a flat kernel given to that variant, this test is where it would show:
    move `metal` into flat_scenes.FLAT then."""
    o_acc, o_cnt = S.oracle_render("metal")
    _, _, _, cornell_variant = render("mix")
    for mode, (info, acc, st, variant) in render_modes(monkeypatch, "metal").items():
        print("metal", mode, "variant", variant, "flat_steps", info.flat_steps, brief(st))
        assert (info.flat_steps > 0) == (mode != "0")
        assert variant != cornell_variant
        assert st["flat_uncertified"] == st["flat_wave_fallbacks"] == st["flat_fallback_hits"] == 0
        assert st["rays"] == o_cnt["rays"]
        assert_oracle_bits(f"metal, RT2_FLAT_BVH={mode}", acc, o_acc, S.decided("metal"))


def test_launch_boundaries_and_a_partition(have_gpu, monkeypatch):
    """`mix` in launches of 5 frames (boundaries inside the 16), and rank 1 of 3 in bands of 2 rows."""
    monkeypatch.delenv("RT2_FLAT_BVH", raising=False)
    o_acc, o_cnt = S.oracle_render("mix")
    mask = S.decided("mix")
    info, full, st, _ = render("mix")
    _, split, st_s, _ = render("mix", launch_frames=5)
    band_h, rank, world = 2, 1, 3
    _, part, st_p, _ = render("mix", partition=(band_h, rank, world))
    rows = local_rows(S.H, band_h, rank, world)
    print("mix full", brief(st), "launches", st["launches"], "; launch_frames 5", brief(st_s), "launches", st_s["launches"],
          "; rank", rank, "of", world, "rows", rows, brief(st_p))
    assert info.flat_steps > 0
    assert_oracle_bits("mix", full, o_acc, mask)
    assert_oracle_bits("mix in launches of 5 frames", split, o_acc, mask)
    assert st_s["launches"] == 4 > st["launches"]  # 5 + 5 + 5 + 1 frames
    assert st_s["rays"] == st["rays"] == o_cnt["rays"]
    assert st_s["flat_uncertified"] == st["flat_uncertified"] >= int(mask.sum())
    assert 0 < len(rows) < S.H and part.shape[0] == len(rows) and st_p["paths"] == len(rows) * S.W * S.FRAMES
    assert np.array_equal(part.view(np.uint32), full[rows].view(np.uint32)), "the partition's rows differ from the full render's"
    assert_oracle_bits("mix, rank 1 of 3", part, o_acc[rows], mask[rows])
    assert int(mask[rows].sum()) <= st_p["flat_uncertified"] <= st["flat_uncertified"]


def test_a_counting_launch_walks_the_bvh_program(have_gpu, monkeypatch):
    """`eight` with enable_stats: the reference's record counters, equal to those of the scene loaded with
    RT2_FLAT_BVH=0; the product kernel's accumulation; no flat counter."""
    monkeypatch.delenv("RT2_FLAT_BVH", raising=False)
    info, acc, st, _ = render("eight", stats=True)
    _, acc_p, st_p, _ = render("eight")
    monkeypatch.setenv("RT2_FLAT_BVH", "0")
    info0, acc0, st0, _ = render("eight", stats=True)
    monkeypatch.delenv("RT2_FLAT_BVH")
    o_acc, o_cnt = S.oracle_render("eight")
    print("eight counting", {k: st[k] for k in ("rays", "bvh_tests", "quad_tests", "xform_visits")}, "oracle", o_cnt)
    assert info.flat_steps > 0 and info0.flat_steps == 0
    for k in ("rays", "bvh_tests", "quad_tests", "xform_visits"):
        assert st[k] == st0[k] > 0, k
    # ... and to the oracle's own: the nodes, quads and transforms the reference's walk visits, slab tests included
    assert (st["rays"], st["bvh_tests"], st["quad_tests"], st["xform_visits"]) == \
        (o_cnt["rays"], o_cnt["bvh"], o_cnt["quad"], o_cnt["xform"])
    assert st["flat_uncertified"] == st["flat_wave_fallbacks"] == st["flat_fallback_hits"] == 0
    assert st_p["flat_uncertified"] > 0  # (the product launch of the same scene did walk the flat program)
    assert np.array_equal(acc.view(np.uint32), acc_p.view(np.uint32)), "counting and product kernels differ"
    assert np.array_equal(acc.view(np.uint32), acc0.view(np.uint32))
    assert_oracle_bits("eight, counting launch", acc, o_acc, S.decided("eight"))


def test_no_inner_node_nothing_to_decide(have_gpu, monkeypatch):
    """`two`: one BVH node over two transformed boxes. D = 0; the oracle's bits in all three modes."""
    check_flat_scene("two", render_modes(monkeypatch, "two"))
