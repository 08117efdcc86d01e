"""The flat walk of small BVHs (rt2_layout.h "Flat program"; DESIGN.md §4 "Flat walk of small BVHs"): the
Cornell-box kernel walks the scene's leaves without the BVH steps' slab tests, certifies per lane that the
reference's slab tests would have changed nothing, and traces the BVH program again for the lanes it cannot
certify. It must change no bit, with the flat program (the default), without it (RT2_FLAT_BVH=0 at scene
load) and with a kernel that certifies no hit (RT2_FLAT_BVH=2: every hit takes the second trace); scenes
that do not qualify keep their BVH walk; the counting kernels keep the reference's record counters.

RT2_FLAT_BVH=2 and the number of hits: neither the oracle nor the counting kernels count hits, so the test
takes them from the flat kernel's own count of the hits its falling-back wave-bounces end with (all hits
under RT2_FLAT_BVH=2, counted from the final hit flags after the second trace) and bounds them from
outside: a path casts at most one ray that misses, so rays - paths <= hits <= rays."""
import pytest

import raytrace2_amd as R
from bits import same_bits
from conftest import scene_path
from helpers import SEED, oracle_render

pytestmark = pytest.mark.gpu


def render(path, w, h, spp, frames, *, stats=False):
    sc = R.Scene(path, SEED)
    tr = R.RayTracer(sc, 0)
    tr.set_seed(SEED)
    tr.SetSamplesPerPixel(spp)
    tr.OnResize((w, h))
    if stats:
        tr.enable_stats(True)
    tr.Render(frames)
    acc = tr.Accumulation().copy()
    st = tr.stats()
    variant = tr.last_launch()["variant"]
    tr.close()
    return sc.info(), acc, st, variant


_oracle = {}


def oracle(name, w, h, spp, frames):
    key = (name, w, h, spp, frames)
    if key not in _oracle:
        acc, _, cnt = oracle_render(name, w, h, spp, frames)
        acc.setflags(write=False)
        _oracle[key] = (acc, cnt)
    return _oracle[key]


@pytest.mark.parametrize("name,w,h", [("cornell_box_original", 128, 128), ("cornell_box2", 64, 64)])
def test_flat_walk_changes_no_bit(have_gpu, monkeypatch, name, w, h):
    spp, frames = 16, 16
    path = scene_path(name)
    o_acc, o_cnt = oracle(name, w, h, spp, frames)
    monkeypatch.delenv("RT2_FLAT_BVH", raising=False)
    info, acc, st, variant = render(path, w, h, spp, frames)
    monkeypatch.setenv("RT2_FLAT_BVH", "0")
    info0, acc0, st0, variant0 = render(path, w, h, spp, frames)
    monkeypatch.setenv("RT2_FLAT_BVH", "2")
    info2, acc2, st2, variant2 = render(path, w, h, spp, frames)
    monkeypatch.delenv("RT2_FLAT_BVH")
    assert variant == variant0 == variant2 == 0  # the Cornell-box kernel
    assert info.flat_steps > 0 and info0.flat_steps == 0 and info2.flat_steps == info.flat_steps
    assert info.flat_steps < info.linear_steps == info0.linear_steps
    print(name, {k: st[k] for k in ("rays", "paths", "flat_uncertified", "flat_wave_fallbacks", "flat_fallback_hits")},
          {k: st2[k] for k in ("rays", "paths", "flat_uncertified", "flat_wave_fallbacks", "flat_fallback_hits")})
    assert same_bits(acc, o_acc), "the flat walk differs from the oracle"
    assert same_bits(acc0, o_acc), "RT2_FLAT_BVH=0 differs from the oracle"
    assert same_bits(acc2, o_acc), "RT2_FLAT_BVH=2 (every hit traced again) differs from the oracle"
    assert st["rays"] == st0["rays"] == st2["rays"] == o_cnt["rays"]
    # the default: some lanes fall back (the slab test is not vacuous), at most 1 % of the rays (a cap)
    assert 0 < st["flat_uncertified"] <= st["rays"] // 100, st
    assert 0 < st["flat_wave_fallbacks"] <= st["flat_uncertified"]
    # without a flat program nothing is counted
    assert st0["flat_uncertified"] == st0["flat_wave_fallbacks"] == st0["flat_fallback_hits"] == 0
    # certifying nothing: every hit is uncertified
    assert st2["flat_uncertified"] == st2["flat_fallback_hits"]
    assert st2["rays"] - st2["paths"] <= st2["flat_uncertified"] <= st2["rays"]


def test_a_scene_that_does_not_qualify_keeps_its_bvh_walk(have_gpu, monkeypatch):
    """cornell_box_volume holds media (a medium's Hit draws random numbers, so visiting one the reference
    culled would shift the stream): no flat program, nothing counted, the oracle's bits."""
    monkeypatch.delenv("RT2_FLAT_BVH", raising=False)
    name, w, h, spp, frames = "cornell_box_volume", 64, 64, 16, 16
    info, acc, st, _ = render(scene_path(name), w, h, spp, frames)
    assert info.flat_steps == 0
    assert st["flat_uncertified"] == st["flat_wave_fallbacks"] == st["flat_fallback_hits"] == 0
    o_acc, o_cnt = oracle(name, w, h, spp, frames)
    assert st["rays"] == o_cnt["rays"] and same_bits(acc, o_acc)


def test_counting_launches_keep_the_reference_counters(have_gpu, monkeypatch):
    """A counting launch of a scene with a flat program walks the BVH program: bvh_tests, quad_tests and
    xform_visits equal those of the scene loaded with RT2_FLAT_BVH=0."""
    name, w, h, spp, frames = "cornell_box_original", 64, 64, 16, 4
    path = scene_path(name)
    monkeypatch.delenv("RT2_FLAT_BVH", raising=False)
    info, acc, st, _ = render(path, w, h, spp, frames, stats=True)
    monkeypatch.setenv("RT2_FLAT_BVH", "0")
    info0, acc0, st0, _ = render(path, w, h, spp, frames, stats=True)
    monkeypatch.delenv("RT2_FLAT_BVH")
    assert info.flat_steps > 0 and info0.flat_steps == 0
    for k in ("rays", "bvh_tests", "quad_tests", "xform_visits"):
        assert st[k] == st0[k] > 0, k
    assert st["flat_uncertified"] == st["flat_wave_fallbacks"] == 0  # (the counting kernel walks no flat program)
    assert same_bits(acc, acc0)
